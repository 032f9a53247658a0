// Anti-instagram colour transform, batched (lf_ai_transform_batch).
//
// Reference: /root/reference/src/anti_instagram/include/anti_instagram/AntiInstagram.py:7-50 calculate_transform() = two
// runKMeans fits (kmeans.py:22-47) on the frame's last 100 rows, the 3- / 4-colour decision, then getparameters2's weighted
// least-squares colour fit (kmeans.py:80-173).
//
// k_ai_kmeans: one workgroup per (frame, fit), grid 2 n.  The fit is km_fit (k_kmeans.h), the arithmetic k_kmeans runs for
// lf_kmeans, so centres, counts, inertia and iterations are bit-identical to lf_kmeans / the oracle given the reference's
// points.  The strip (the frame's last S = min(rows, 100) rows) is contiguous in the frame, so the kernel reads it in place, in
// raster order, and every load coalesces; all sums are order-free integer sums.  The reference's column-major point order
// (getimgdatapts: point col S + row) matters only in the re-seed tie-break, where KmStripOrder supplies it.
//
// k_ai_fit: one thread per frame, f64.  getparameters2's 15 x 6 system solved by Householder QR (the system's condition number is
// ~1e4 on camera frames; the normal equations would lose ~1e-10 in p), cost = |(Q^T b)[6:15]|^2, the residual sum of squares
// np.linalg.lstsq reports.  The library builds with -ffp-contract=off: every product and sum below rounds on its own.
#include "k_kmeans.h"

namespace lf {

// kmeans.py:9-10 (B, G, R): fit 0 = CENTERS2 (dark grey, red, yellow, white), fit 1 = CENTERS (dark grey, yellow, white)
__constant__ double c_ai_init4[12] = { 60, 60, 60, 60, 60, 240, 50, 240, 240, 240, 240, 240 };
__constant__ double c_ai_init3[9] = { 60, 60, 60, 50, 240, 240, 240, 240, 240 };

// raster position i = row cols + col  <->  the reference's column-major index col S + row
struct KmStripOrder {
    int S, cols;
    __device__ __forceinline__ int key(int i) const { return (i % cols) * S + i / cols; }
    __device__ __forceinline__ int pos(int key) const { return (key % S) * cols + key / S; }
};

// per (frame, fit) b = 2 f + fit: fo [b][16] (centres, inertia at [3k]), fc [b][4] counts, fs [b] iterations or -1
__global__ __launch_bounds__(KM_T) void k_ai_kmeans(const uint8_t* __restrict__ strips, long long frame_stride, int S, int cols,
                                                    uint8_t* __restrict__ lab, double* __restrict__ fo, long long* __restrict__ fc,
                                                    int* __restrict__ fs)
{
    const int b = blockIdx.x, f = b >> 1, fit = b & 1;
    const int n = S * cols;
    km_fit(strips + (size_t)f * frame_stride, n, fit ? 3 : 4, fit ? c_ai_init3 : c_ai_init4, 25, 1e-4, lab + (size_t)b * n,
           fo + 16 * (size_t)b, fc + 4 * (size_t)b, fs + b, KmStripOrder{ S, cols });
}

// Householder QR least squares of A [15][6] p = y: p, and the residual sum of squares |(Q^T y)[6:]|^2
__device__ void ai_lstsq(double (&A)[15][6], double (&y)[15], double (&p)[6], double* rss)
{
    for (int j = 0; j < 6; ++j) {
        double sub = 0.0;
        for (int i = j + 1; i < 15; ++i) sub += A[i][j] * A[i][j];
        const double nrm = dm::dsqrt(A[j][j] * A[j][j] + sub);
        const double alpha = A[j][j] > 0.0 ? -nrm : nrm;         // the sign that avoids cancellation in v0
        const double v0 = A[j][j] - alpha;                       // v = (v0, A[j+1..14][j])
        const double vv = v0 * v0 + sub;
        if (nrm == 0.0 || vv == 0.0) continue;
        for (int c = j + 1; c < 6; ++c) {
            double d = v0 * A[j][c];
            for (int i = j + 1; i < 15; ++i) d += A[i][j] * A[i][c];
            const double t = 2.0 * d / vv;
            A[j][c] -= t * v0;
            for (int i = j + 1; i < 15; ++i) A[i][c] -= t * A[i][j];
        }
        {
            double d = v0 * y[j];
            for (int i = j + 1; i < 15; ++i) d += A[i][j] * y[i];
            const double t = 2.0 * d / vv;
            y[j] -= t * v0;
            for (int i = j + 1; i < 15; ++i) y[i] -= t * A[i][j];
        }
        A[j][j] = alpha;
    }
    for (int j = 5; j >= 0; --j) {
        double s = y[j];
        for (int c = j + 1; c < 6; ++c) s -= A[j][c] * p[c];
        p[j] = s / A[j][j];
    }
    double r = 0.0;
    for (int i = 6; i < 15; ++i) r += y[i] * y[i];
    *rss = r;
}

__global__ __launch_bounds__(64) void k_ai_fit(int n_frames, const double* __restrict__ fo, const long long* __restrict__ fc,
                                               const int* __restrict__ fs, lf_ai_transform* __restrict__ out)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_frames) return;
    lf_ai_transform r = {};
    const int b4 = 2 * f, b3 = 2 * f + 1;
    if (fs[b4] < 0 || fs[b3] < 0) { r.status = LF_ERR_BAD_ARG; out[f] = r; return; }
    r.n_iter4 = fs[b4]; r.n_iter3 = fs[b3];
    const double* o4 = fo + 16 * (size_t)b4; const double* o3 = fo + 16 * (size_t)b3;
    r.score4 = -o4[12]; r.score3 = -o3[9];
    // AntiInstagram.py:16-33: the 4-colour fit keeps rows 0, 2, 3 (the red cluster is dropped)
    const bool three = (r.score3 + 3e7) > r.score4;
    r.n_colors = three ? 3 : 4;
    double tr[3][3], tv[3][3], w[3];
    long long cnt[3];
    for (int i = 0; i < 3; ++i) {
        const int src = three ? i : (i == 0 ? 0 : i + 1);
        for (int c = 0; c < 3; ++c) {
            tr[i][c] = three ? o3[3 * i + c] : o4[3 * src + c];
            tv[i][c] = three ? c_ai_init3[3 * i + c] : c_ai_init4[3 * src + c];
            r.centers[i][c] = tr[i][c];
        }
        cnt[i] = three ? fc[4 * (size_t)b3 + i] : fc[4 * (size_t)b4 + src];
        r.counts[i] = cnt[i];
    }
    // kmeans.py:120-140: weights = counts / sum(counts); rows 0-8 colour terms, 9-11 the diagonal prior, 12-14 the scale prior
    const double sw = (double)(cnt[0] + cnt[1] + cnt[2]);
    for (int i = 0; i < 3; ++i) w[i] = (double)cnt[i] / sw;
    double A[15][6], y[15], p[6];
    for (int i = 0; i < 15; ++i) { y[i] = 0.0; for (int c = 0; c < 6; ++c) A[i][c] = 0.0; }
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 3; ++i) {
            A[3 * c + i][2 * c] = w[i] * tr[i][c];
            A[3 * c + i][2 * c + 1] = w[i];
            y[3 * c + i] = w[i] * tv[i][c];
        }
    A[9][0] = 300.0; A[9][2] = -300.0;
    A[10][2] = 300.0; A[10][4] = -300.0;
    A[11][0] = 300.0; A[11][4] = -300.0;
    for (int c = 0; c < 3; ++c) { A[12 + c][2 * c] = 0.2; y[12 + c] = 0.2; }
    double cost;
    ai_lstsq(A, y, p, &cost);
    if (p[0] < 0.0 || p[2] < 0.0 || p[4] < 0.0) cost += 1000000.0;     // INFEASIBILITY_PENALTY (kmeans.py:150-151)
    r.status = LF_OK;
    r.success = p[0] != 0.0;                                           // AntiInstagram.py:39-41
    // kmeans.py:173 returns (ch0, ch2, ch1); calculate_transform reads them as r, g, b
    r.scale[0] = p[0]; r.scale[1] = p[4]; r.scale[2] = p[2];
    r.shift[0] = p[1]; r.shift[1] = p[5]; r.shift[2] = p[3];
    r.cost = cost;
    r.health = r.success ? 1.0 / (cost + 2.220446049250313e-16) : 0.0;  // 1 / (cost + np.finfo('double').eps)
    if (!r.success) { for (int c = 0; c < 3; ++c) { r.scale[c] = 0.0; r.shift[c] = 0.0; } }
    out[f] = r;
}

void launch_ai_transform(const uint8_t* strips, long long frame_stride, int n_frames, int S, int cols, uint8_t* lab, double* fo,
                         long long* fc, int* fs, lf_ai_transform* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_ai_kmeans, dim3(2 * n_frames), dim3(KM_T), 0, s, strips, frame_stride, S, cols, lab, fo, fc, fs);
    hipLaunchKernelGGL(k_ai_fit, dim3((n_frames + 63) / 64), dim3(64), 0, s, n_frames, fo, fc, fs, out);
}

}  // namespace lf
