// A batch's trajectory smoothed against the live map (k_map_smooth.hip, lanefront_map_smooth.hip): include/lanefront.h
// "lf_map_smooth" is the contract, tests/map_smooth_ref.py its sequential restatement.  Shared by the kernels and the host side.
#pragma once
#include "k_map_align.h"

namespace lf {
namespace ms {

constexpr int kSolveThreads = 256;         // the workgroup of one chain's solve

// one pose of a chain in the block tridiagonal system, as the reduction leaves it: D's upper triangle (00 01 02 11 12 22), the
// right-hand side, the coupling C = H[i, i - h] to the lower neighbour of the node's level (row major), the multipliers
// y = D^-1 b, P = D^-1 C, Q = D^-1 C[i + h]^T of the level that eliminated it, and the step t
struct Node { double D[6], b[3], C[9], y[3], P[9], Q[9], t[3]; };

struct Chain { int32_t stopped, status, iterations, reserved; };

// device arrays of one call beside ma::Batch's.  ma::Batch::res holds the state between the launches: x, y, theta are the
// iterate, status is 1 while the frame had a map factor in the last iteration evaluated (the last solve writes the real one)
struct Batch {
    ma::Batch a;
    const int32_t* chain_offset;           // [n_chains + 1]
    const int32_t* chain_of;               // [n_frames]: the chain of a frame
    int n_chains;
    double* sums;                          // [n_frames][9]: N00 N01 N02 N11 N12 N22 g0 g1 g2 of the frame's map factor, +0 without one
    Node* node;                            // [n_frames]
    Chain* chain;                          // [n_chains], zero before iteration 0
    int32_t* chain_status;                 // [n_chains]
};

// iteration k of every chain that has not stopped: the sums (one wave per frame), then the solve (one workgroup per chain); the
// solve of the last iteration also tests the limits and writes the results
void launch_smooth_iteration(const lf_smooth_config& c, const MapDevice& md, const Batch& b, int k, hipStream_t s);

}  // namespace ms
}  // namespace lf
