// TEST HARNESS ONLY -- not part of the product.
// lane_slam_amd/csrc/nfa.h compiled for the host: both forms of the product's NFA, for tests/test_nfa_cpu.py.
#define LF_HOST_SIM 1
#include "../../lane_slam_amd/csrc/nfa.h"

extern "C" double nfa_log_gamma_first(int n, int k, double p, double log_nt) { return lf::nfa_tail<false>(n, k, p, log_nt); }     // EDLines
extern "C" double nfa_plain_first(int n, int k, double p, double log_nt) { return lf::nfa_tail<true>(n, k, p, log_nt); }         // LSD
