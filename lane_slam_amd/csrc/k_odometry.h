// Odometry (include/lanefront_odometry.h): what k_odometry.hip and its host side (lanefront_odometry.hip) share.
#pragma once
#include "common.h"
#include "../../include/lanefront_odometry.h"

namespace lf {

enum OdoStage { ODO_PREPARE = 0, ODO_HEADING, ODO_TERMS, ODO_POSITION, ODO_SAMPLE, ODO_N_STAGES };

constexpr uint8_t kOdoDriven = 1, kOdoTurn = 2;      // a command's flags

// One step's arrays on the device.  The commands are grouped by stream, each stream's in arrival order: position p of the
// grouped order holds the command orig[p] of the caller's arrays, and stream s owns the positions [offset[s], offset[s + 1]).
struct OdoStep {
    int n_commands, n_frames, n_streams;
    double wheel_distance, dt_max;
    int stamp_full, flip_y;
    // uploaded
    const long long* stamp;         // [n_commands]
    const double* vl; const double* vr;
    const int* orig; const int* cstream;
    const int* offset;              // [n_streams + 1]
    const long long* fstamp;        // [n_frames]
    const int* fstream;
    // between the stages
    uint8_t* flags;                 // kOdoDriven | kOdoTurn
    double* a; double* sa; double* ca;     // the turn angle, its sine and cosine
    double* rk;                     // r of a turning command, k of a straight one
    double* heading;                // theta before the command
    double* t0; double* t1;         // r*sin, r*cos of the heading (turning) or k*cos, k*(-sin) (straight)
    double* pose;                   // [n_commands][3] after the command, the state's own y
    lf_odometry_state* state;       // [n_streams]
    double* start;                  // [n_streams][3] the pose at the start of the call
    // the caller's outputs (device addresses), in the caller's order; flip_y applied
    double* frame_pose; int* frame_cmd; double* trajectory; uint8_t* driven;
};

void launch_odo_prepare(const OdoStep& o, hipStream_t s);
void launch_odo_heading(const OdoStep& o, hipStream_t s);
void launch_odo_terms(const OdoStep& o, hipStream_t s);
void launch_odo_position(const OdoStep& o, hipStream_t s);
void launch_odo_sample(const OdoStep& o, hipStream_t s);

}  // namespace lf
