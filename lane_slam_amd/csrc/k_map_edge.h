// The device statements of an SE(2) relative-pose factor that lf_map_smooth and lf_map_graph_solve share (include/lanefront.h
// "lf_map_smooth" states them: "edge f -> n" and "solve3"): the Jacobians at the iterate, the products A^T W B and A^T W e, a
// node's share of a factor, the dot of two 3-vectors and the 3 x 3 solve.  k_map_smooth.hip and k_map_graph.hip include it and
// run the same statements; both are built with -ffp-contract=off.
#pragma once
#include "k_map_pairs.h"

namespace lf {
namespace me {

// (A^T W B)[r][c] and (A^T W e)[r] for row-major 3 x 3 A, B and the diagonal W, in the contract's order
__device__ __forceinline__ double atwb(const double* A, const double* w, const double* B, int r, int c)
{
    return ((A[r] * w[0]) * B[c] + (A[3 + r] * w[1]) * B[3 + c]) + (A[6 + r] * w[2]) * B[6 + c];
}
__device__ __forceinline__ double atwe(const double* A, const double* w, const double* e, int r)
{
    return ((A[r] * w[0]) * e[0] + (A[3 + r] * w[1]) * e[1]) + (A[6 + r] * w[2]) * e[2];
}
__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// the Jacobians of the edge f -> n at the iterate: (s, c) = sin, cos of th_f, (px, py) = n's position in f's frame
__device__ __forceinline__ void jacobians(double s, double c, double px, double py, double* Jf, double* Jn)
{
    Jf[0] = -c; Jf[1] = -s; Jf[2] = py;
    Jf[3] = s; Jf[4] = -c; Jf[5] = -px;
    Jf[6] = 0.0; Jf[7] = 0.0; Jf[8] = -1.0;
    Jn[0] = c; Jn[1] = s; Jn[2] = 0.0;
    Jn[3] = -s; Jn[4] = c; Jn[5] = 0.0;
    Jn[6] = 0.0; Jn[7] = 0.0; Jn[8] = 1.0;
}

// D += A^T W A (upper triangle), b -= A^T W e
__device__ __forceinline__ void add_factor(double* D, double* b, const double* A, const double* w, const double* e)
{
    D[0] = D[0] + atwb(A, w, A, 0, 0); D[1] = D[1] + atwb(A, w, A, 0, 1); D[2] = D[2] + atwb(A, w, A, 0, 2);
    D[3] = D[3] + atwb(A, w, A, 1, 1); D[4] = D[4] + atwb(A, w, A, 1, 2);
    D[5] = D[5] + atwb(A, w, A, 2, 2);
    b[0] = b[0] - atwe(A, w, e, 0); b[1] = b[1] - atwe(A, w, e, 1); b[2] = b[2] - atwe(A, w, e, 2);
}

// the contract's solve3(D, v): the LDL^T of D's upper triangle (00 01 02 11 12 22) with its pivot test, then t; false: it failed
__device__ __forceinline__ bool solve3(const double* D, const double* v, double* t)
{
    ma::Ldl f;
    return ma::ldl_factor(D[0], D[1], D[2], D[3], D[4], D[5], f) && ma::ldl_apply(f, v[0], v[1], v[2], t[0], t[1], t[2]);
}

}  // namespace me
}  // namespace lf
