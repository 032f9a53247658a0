/* lanefront -- odometry on the device: wheel commands to frame poses, batched.
 *
 * The device form of the reference's odometry node (src/odometry/src/odometry.py, the `map -> duck` tf that show_map builds the
 * map with): differential-drive dead reckoning from WheelsCmdStamped messages.  The node takes one message per call; here a whole
 * log's commands, for up to LF_ODOMETRY_MAX_STREAMS robots at once, are integrated in one call and sampled at the frames' stamps,
 * which gives the `frame_pose` rows lf_map_step*, lf_map_align, lf_map_smooth and lf_map_graph_solve take.
 *
 * A header of its own: include/lanefront.h and lf_abi_version() are unchanged.  Error codes and LF_API are lanefront.h's.
 *
 * Semantics (tests/odometry_ref.py is the statement, bit for bit).  Per stream the state is x, y, theta, last_t (f64) and
 * last_stamp_ns (i64).  Per command (stamp_ns, Vl, Vr), in arrival order within its stream:
 *   t  = (double)(stamp_ns % 1000000000) / 1e9
 *   dt = t - last_t                                   LF_ODOMETRY_STAMP_NSECS (default; odometry.py:111-112 reads only the
 *                                                     nanosecond field, so dt is negative once per second and that command is
 *                                                     skipped -- the reference's quirk, kept)
 *      = (double)(stamp_ns - last_stamp_ns) / 1e9     LF_ODOMETRY_STAMP_FULL
 *   last_t = t, last_stamp_ns = stamp_ns              always
 *   driven iff dt > 0.0 && dt < dt_max                (:113)
 *   driven, Vl == Vr (:76-78):   k = dt*Vl;  x = x + k*cos(theta);  y = y + k*(-sin(theta));  theta untouched (-0.0 stays -0.0)
 *   driven otherwise (:81-100, rotate_point :12-23; l = wheel_distance), every operation rounded on its own, no FMA:
 *       w = (Vr-Vl)/l;  r = (l*(Vl+Vr))/(2*(Vl-Vr));  a = w*dt
 *       cx = x + r*sin(theta);  cy = y + r*cos(theta);  dx = x - cx;  dy = y - cy
 *       ndx = dx*cos(a) + dy*sin(a);  ndy = dy*cos(a) - dx*sin(a)
 *       x = cx + ndx;  y = cy + ndy;  theta = theta + a
 * sin and cos are the library's deterministic routines (csrc/detmath.h dsincos; within 1 - 2 ulp of libm for |theta| <= 1e6 rad).
 *
 * flip_y (default 0) negates y in every OUTPUT (frame poses, trajectory, lf_odometry_get_state) and never touches the state.  The
 * reference moves along (cos theta, -sin theta) and turns clockwise for Vr > Vl, yet publishes (x, y, theta) as a standard yaw;
 * (x, -y, theta) is the consistent right-handed pose for lf_map_*.  A parity knob, like lf_config.lsd_seed_order.
 *
 * Frames.  A frame (frame_stamp_ns, stream) gets its stream's pose after the last command of THIS call, in the stream's order,
 * whose stamp_ns <= frame_stamp_ns (a zero-order hold: what a tf lookup of the latest transform gives), and that command's index in
 * the call's arrays in frame_cmd; with no such command it gets the stream's pose at the start of the call and frame_cmd -1.  Frames
 * need not be sorted.
 *
 * LF_ERR_BAD_ARG, with a message that names the index: a negative stamp; stamps that decrease within a stream or start below the
 * stream's last_stamp_ns; a velocity that is not finite; a stream out of range; a wheel_distance or dt_max that is not finite or is
 * <= 0; a stamp_mode other than the two.  LF_ERR_CAPACITY: counts above what lf_odometry_create was given.  A refused call leaves
 * the state as it was.  n_commands == 0 (pure sampling) and n_frames == 0 (pure integration) are legal.
 */
#ifndef LANEFRONT_ODOMETRY_H
#define LANEFRONT_ODOMETRY_H

#include "lanefront.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lf_odometry lf_odometry;

typedef struct lf_odometry_config {
    double wheel_distance;     /* l of the reference's drive(): 0.5 */
    double dt_max;             /* commands further apart than this are not driven: 0.3 */
    int32_t stamp_mode;        /* LF_ODOMETRY_STAMP_NSECS (the reference) or LF_ODOMETRY_STAMP_FULL */
    int32_t flip_y;            /* outputs carry -y */
} lf_odometry_config;          /* 24 bytes */

typedef struct lf_odometry_state {
    double x, y, theta, last_t;
    int64_t last_stamp_ns;
    int64_t n_commands, n_driven;      /* since the stream's last reset */
} lf_odometry_state;           /* 56 bytes */

#define LF_ODOMETRY_STAMP_NSECS 0
#define LF_ODOMETRY_STAMP_FULL 1
#define LF_ODOMETRY_MAX_STREAMS 4096

LF_API void lf_odometry_default_config(lf_odometry_config* cfg);
/* n_streams in [1, LF_ODOMETRY_MAX_STREAMS], max_commands in [1, 1 << 22], max_frames in [1, 1 << 22]: the most one step takes */
LF_API int lf_odometry_create(int device_id, const lf_odometry_config* cfg, int n_streams, int max_commands, int max_frames, lf_odometry** out);
LF_API void lf_odometry_destroy(lf_odometry* od);
/* od NULL: the last failure of lf_odometry_create */
LF_API const char* lf_odometry_last_error(const lf_odometry* od);
/* stream -1: every stream; state NULL: zeros.  The state is taken as it is (y is the state's own, whatever flip_y says); one that is
 * not finite, or whose last_stamp_ns or a counter is negative, is LF_ERR_BAD_ARG.  Waits for queued work. */
LF_API int lf_odometry_reset(lf_odometry* od, int stream, const lf_odometry_state* state_or_null);
/* waits for queued work */
LF_API int lf_odometry_get_state(lf_odometry* od, int stream, lf_odometry_state* state);
/* Inputs are host arrays.  cmd_stream / frame_stream NULL: stream 0.  frame_pose [n_frames][3] (x, y, theta), frame_cmd [n_frames],
 * trajectory [n_commands][3] (the command's stream after it) and driven [n_commands] are host arrays (out_on_device 0: the call
 * returns when they are in place) or device arrays (1: the call is queued on the handle's stream; lf_odometry_synchronize waits). */
LF_API int lf_odometry_step(lf_odometry* od, int n_commands, const int64_t* stamp_ns, const double* vel_left, const double* vel_right,
                            const int32_t* cmd_stream_or_null, int n_frames, const int64_t* frame_stamp_ns,
                            const int32_t* frame_stream_or_null, double* frame_pose, int32_t* frame_cmd_or_null,
                            double* trajectory_or_null, uint8_t* driven_or_null, int out_on_device);
LF_API int lf_odometry_synchronize(lf_odometry* od);
LF_API int lf_odometry_set_profiling(lf_odometry* od, int on);
/* ms accumulated and launches counted per stage since the last call (resets both); the stages, in order: k_odo_prepare,
 * k_odo_heading, k_odo_terms, k_odo_position, k_odo_sample */
LF_API int lf_odometry_get_timing(lf_odometry* od, double* ms, int32_t* launches, int n_stages);

#ifdef __cplusplus
}
#endif

#endif
