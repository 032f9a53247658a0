// Loop-closure candidates among stored key frames (k_places.hip, lanefront_places.hip): include/lanefront_places.h is the contract,
// tests/places_ref.py its sequential restatement.  Shared by the kernels and the host side.
#pragma once
#include "../../include/lanefront_places.h"
#include "k_frame_motion.h"

namespace lf {

// lanefront_motion.hip: why lf_motion_estimate refuses the configuration, or null
const char* motion_bad_config(const lf_motion_config* c);

namespace pc {

constexpr int kThreads = 256;              // k_places_score: four waves, each with keys of its own; k_places_top: one workgroup per query
constexpr int kWaves = kThreads / 64;
constexpr int kKeysPerBlock = 32;          // keys of one workgroup of k_places_score: the query frame's codes stay in registers over them
constexpr int kTurn = 64;                  // segments of a frame a wave holds at a time, one per lane
constexpr int kQueryInts = 4;              // per query: q0, q1 (the frame's segment range, clamped by the host), the visible keys, 0
constexpr int kGatherInts = 3;             // per copy: the first source segment, the segments, the first destination segment
static_assert(LF_PLACES_MAX_TOP_K == 16 && LF_PLACES_MAX_KEYS == 1 << 16 && LF_PLACES_MAX_SEGMENTS == 1 << 24, "lanefront_places.h states these");
static_assert(LF_PLACES_MAX_SCORES == 1 << 26 && LF_PLACES_MAX_QUERIES == ma::kMaxFrames, "lanefront_places.h states these");

// the store's device arrays: key k holds the segments key_offset[k] <= j < key_offset[k + 1]; 0 = key_offset[0] <= ... <= key_offset[count]
// <= the arrays' length by construction (lanefront_places.hip writes them)
struct Store {
    int* key_offset; double* ground; uint8_t* color; uint8_t* keep; uint8_t* code;
    int count;
};

// a batch's device arrays; color and keep may be null
struct Frames {
    const double* ground; const uint8_t* color; const uint8_t* keep; const uint8_t* code;
};

struct Query {
    Store store;
    Frames frames;
    const int* job;                        // [n_queries][kQueryInts]
    int* score;                            // [n_queries][store.count]
    lf_place_hit* hits;                    // [n_queries][top_k]
    int n_queries;
};

// k_places_score then k_places_top on the stream
void launch_places_score(const lf_places_config& c, const Query& q, hipStream_t s);
void launch_places_top(const lf_places_config& c, const Query& q, hipStream_t s);
// n_jobs copies of whole frames from a batch's arrays into the store's: a null color is stored as 0, a null keep as 1
void launch_places_gather(const Frames& from, const Store& to, const int* job, int n_jobs, hipStream_t s);

}  // namespace pc
}  // namespace lf
