// Anti-instagram colour clustering (k-means part).
//
// Reference: /root/reference/src/anti_instagram/include/anti_instagram/kmeans.py:14-47 -- runKMeans() =
// sklearn.cluster.KMeans(n_clusters, max_iter = 25, init = <array>).fit_predict on the B, G, R pixels of the frame's last
// 100 rows, then cluster_centers_, the label counts and score() = -inertia.  Arithmetic: scikit-learn's Lloyd iteration
// (centred data, tolerance = 1e-4 x mean feature variance, strict-convergence test on the labels, empty clusters re-seeded
// with the farthest samples), restated in oracle/lf_oracle_kmeans.c, which is pinned against the reference's own function
// (tests/golden/kmeans.npz).  This kernel computes the SAME fixed arithmetic as the oracle, so the two agree bit for bit:
// distances as csq + (-2 fma(x2, c2, fma(x1, c1, x0 c0))) (what the BLAS product gives, ties included), every sum over
// samples as an exact integer sum (order free: LDS atomics), the handful of float64 operations per iteration by one thread.
//
// One workgroup of 1024 threads runs the whole fit: a frame's strip is 16 000 .. 192 000 points, a Lloyd iteration over it
// a few microseconds, and the iterations are strictly sequential -- there is nothing for a second workgroup to do.
#include "k_kmeans.h"

namespace lf {

__global__ __launch_bounds__(KM_T) void k_kmeans(const uint8_t* __restrict__ bgr, int n, int k, const double* __restrict__ init,
                                                 int max_iter, double tol_rel, uint8_t* __restrict__ lab, double* __restrict__ out,
                                                 long long* __restrict__ counts, int* __restrict__ status)
{
    km_fit(bgr, n, k, init, max_iter, tol_rel, lab, out, counts, status, KmIdentityOrder());
}

void launch_kmeans(const uint8_t* bgr, int n, int k, const double* init, int max_iter, double tol_rel, uint8_t* lab, double* out,
                   long long* counts, int* status, hipStream_t s)
{
    hipLaunchKernelGGL(k_kmeans, dim3(1), dim3(KM_T), 0, s, bgr, n, k, init, max_iter, tol_rel, lab, out, counts, status);
}

}  // namespace lf
