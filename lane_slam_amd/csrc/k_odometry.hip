// Odometry (include/lanefront_odometry.h; the reference's odometry.py getPose / drive / rotate_point): one step's commands, grouped
// by stream, to per-command poses and per-frame samples.
//
// getPose sets last_t on every message whether it drives or not, so dt, the gate, w, r, the turn angle a and sin / cos of a are
// per command (k_odo_prepare, grid-wide).  The heading is a chain of plain f64 additions (k_odo_heading, one wave per stream, one
// lane walking LDS).  With the headings, sin / cos of each and the products r*sin, r*cos, k*cos, k*(-sin) are per command again
// (k_odo_terms).  What stays serial is the position: a few dependent adds and multiplies per command (k_odo_position, one wave per
// stream).  k_odo_sample holds each frame's pose (one lane per frame, a bounded binary search).
//
// Every f64 operation is the statement's, rounded on its own (-ffp-contract=off); sin and cos are detmath.h's dsincos.
#include "k_odometry.h"

namespace lf {

constexpr int kOdoThreads = 256;     // the grid-wide kernels
constexpr int kOdoChunk = 64;        // commands a wave stages in LDS at a time: one per lane
constexpr int kOdoSearchSteps = 23;  // halvings that empty a range of up to 1 << 22 commands

__device__ __forceinline__ double odo_time_of(long long stamp) { return (double)(stamp % 1000000000LL) / 1e9; }

__global__ void __launch_bounds__(kOdoThreads) k_odo_prepare(OdoStep o)
{
    const int p = blockIdx.x * kOdoThreads + threadIdx.x;
    if (p >= o.n_commands) return;
    const int s = o.cstream[p];
    const bool first = p == o.offset[s];                 // its predecessor is the state
    const long long st = o.stamp[p];
    double dt;
    if (o.stamp_full) {
        const long long prev = first ? (long long)o.state[s].last_stamp_ns : o.stamp[p - 1];
        dt = (double)(st - prev) / 1e9;
    } else {
        const double last_t = first ? o.state[s].last_t : odo_time_of(o.stamp[p - 1]);
        dt = odo_time_of(st) - last_t;
    }
    const double vl = o.vl[p], vr = o.vr[p], l = o.wheel_distance;
    const bool driven = dt > 0.0 && dt < o.dt_max, turn = vl != vr;
    // a command that does not turn the robot carries the angle -0.0: theta + (-0.0) is theta, bit for bit, for every theta (a -0.0
    // heading stays -0.0), so neither chain needs to ask
    double a = -0.0, sa = 0.0, ca = 1.0, rk = dt * vl;
    if (turn) {
        const double w = (vr - vl) / l;
        rk = (l * (vl + vr)) / (2.0 * (vl - vr));
        if (driven) { a = w * dt; dm::dsincos(a, sa, ca); }
    }
    o.flags[p] = (uint8_t)((driven ? kOdoDriven : 0) | (turn ? kOdoTurn : 0));
    o.a[p] = a; o.sa[p] = sa; o.ca[p] = ca; o.rk[p] = rk;
}

// One wave per stream.  The wave loads 64 commands' turn angles, one per lane, and parks them in LDS; lane 0 walks them
// with one f64 add per command (-0.0 where the robot does not turn) and leaves the heading BEFORE each command in LDS; the wave
// writes those out coalesced.  The next 64 are loaded (into registers) before the walk starts and stored after it.  A chunk's
// unused tail carries -0.0, so the walk's trip count is fixed.
__global__ void __launch_bounds__(kOdoChunk) k_odo_heading(OdoStep o)
{
    __shared__ double s_a[kOdoChunk], s_h[kOdoChunk];
    const int s = blockIdx.x, lane = threadIdx.x;
    const int b = o.offset[s], n = o.offset[s + 1] - b;
    if (n <= 0) return;
    const int chunks = (n + kOdoChunk - 1) / kOdoChunk;
    double theta = o.state[s].theta;
    double a = -0.0;
    if (lane < n) a = o.a[b + lane];
    for (int c = 0; c < chunks; ++c) {
        s_a[lane] = a;
        __syncthreads();
        const int nx = (c + 1) * kOdoChunk + lane;
        a = -0.0;
        if (nx < n) a = o.a[b + nx];
        if (lane == 0) {
#pragma unroll 8
            for (int j = 0; j < kOdoChunk; ++j) {
                s_h[j] = theta;
                theta = theta + s_a[j];
            }
        }
        __syncthreads();
        const int i = c * kOdoChunk + lane;
        if (i < n) o.heading[b + i] = s_h[lane];
    }
}

__global__ void __launch_bounds__(kOdoThreads) k_odo_terms(OdoStep o)
{
    const int p = blockIdx.x * kOdoThreads + threadIdx.x;
    if (p >= o.n_commands) return;
    const uint8_t f = o.flags[p];
    double t0 = -0.0, t1 = -0.0;         // (an undriven command moves x and y by -0.0: they keep every bit)
    if (f & kOdoDriven) {
        double sn, cs;
        dm::dsincos(o.heading[p], sn, cs);
        const double rk = o.rk[p];
        if (f & kOdoTurn) { t0 = rk * sn; t1 = rk * cs; }
        else { t0 = rk * cs; t1 = rk * (-sn); }
    }
    o.t0[p] = t0; o.t1[p] = t1;
}

// One wave per stream, every stream (one without commands only reports where it stands).  Staged like k_odo_heading; lane 0 does
// the dependent chain from the precomputed terms.  x + t0 and y + t1 are the centre of curvature of a turn and the new position of
// a straight command alike, and of an undriven command they are x and y themselves (its terms are -0.0), so the walk has no branch
// and one choice: a driven turn adds the rotated offset.
__global__ void __launch_bounds__(kOdoChunk) k_odo_position(OdoStep o)
{
    __shared__ double s_t0[kOdoChunk], s_t1[kOdoChunk], s_sa[kOdoChunk], s_ca[kOdoChunk], s_x[kOdoChunk], s_y[kOdoChunk];
    __shared__ uint8_t s_f[kOdoChunk];
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= o.n_streams) return;
    const int b = o.offset[s], n = o.offset[s + 1] - b;
    lf_odometry_state st = o.state[s];
    double x = st.x, y = st.y;
    if (lane == 0) { o.start[3 * s] = x; o.start[3 * s + 1] = y; o.start[3 * s + 2] = st.theta; }
    if (n <= 0) return;
    const int chunks = (n + kOdoChunk - 1) / kOdoChunk;
    long long n_driven = 0;
    double t0 = -0.0, t1 = -0.0, sa = 0.0, ca = 1.0, a = -0.0, h = 0.0;
    uint8_t f = 0;
    if (lane < n) {
        const int p = b + lane;
        t0 = o.t0[p]; t1 = o.t1[p]; sa = o.sa[p]; ca = o.ca[p]; a = o.a[p]; h = o.heading[p]; f = o.flags[p];
    }
    for (int c = 0; c < chunks; ++c) {
        s_t0[lane] = t0; s_t1[lane] = t1; s_sa[lane] = sa; s_ca[lane] = ca; s_f[lane] = f;
        const double a_c = a, h_c = h;
        const uint8_t f_c = f;
        __syncthreads();
        const int nx = (c + 1) * kOdoChunk + lane;
        f = 0; t0 = -0.0; t1 = -0.0;
        if (nx < n) {
            const int p = b + nx;
            t0 = o.t0[p]; t1 = o.t1[p]; sa = o.sa[p]; ca = o.ca[p]; a = o.a[p]; h = o.heading[p]; f = o.flags[p];
        }
        if (lane == 0) {
#pragma unroll 8
            for (int j = 0; j < kOdoChunk; ++j) {
                const uint8_t fj = s_f[j];
                const double cx = x + s_t0[j], cy = y + s_t1[j];
                const double dx = x - cx, dy = y - cy;
                const double ndx = dx * s_ca[j] + dy * s_sa[j], ndy = dy * s_ca[j] - dx * s_sa[j];
                const double xt = cx + ndx, yt = cy + ndy;
                const bool arc = fj == (kOdoDriven | kOdoTurn);
                x = arc ? xt : cx;
                y = arc ? yt : cy;
                n_driven += fj & kOdoDriven;
                s_x[j] = x; s_y[j] = y;
            }
        }
        __syncthreads();
        const int i = c * kOdoChunk + lane;
        if (i < n) {
            const int p = b + i;
            const double px = s_x[lane], py = s_y[lane];
            const double th = h_c + a_c;          // the add k_odo_heading made
            o.pose[3 * (size_t)p] = px; o.pose[3 * (size_t)p + 1] = py; o.pose[3 * (size_t)p + 2] = th;
            const size_t q = (size_t)o.orig[p];
            if (o.trajectory) { o.trajectory[3 * q] = px; o.trajectory[3 * q + 1] = o.flip_y ? -py : py; o.trajectory[3 * q + 2] = th; }
            if (o.driven) o.driven[q] = f_c & kOdoDriven;
            if (i == n - 1) {                    // the stream's last command: the new state, but for what lane 0 holds
                o.state[s].theta = th;
                o.state[s].last_t = odo_time_of(o.stamp[p]);
                o.state[s].last_stamp_ns = o.stamp[p];
                o.state[s].n_commands = st.n_commands + n;
            }
        }
    }
    if (lane == 0) { o.state[s].x = x; o.state[s].y = y; o.state[s].n_driven = st.n_driven + n_driven; }
}

__global__ void __launch_bounds__(kOdoThreads) k_odo_sample(OdoStep o)
{
    const int f = blockIdx.x * kOdoThreads + threadIdx.x;
    if (f >= o.n_frames) return;
    const int s = o.fstream[f];
    const long long fs = o.fstamp[f];
    const int b = o.offset[s];
    int lo = b, hi = o.offset[s + 1];        // the first command of the stream with a stamp above the frame's is in [lo, hi]
    for (int it = 0; it < kOdoSearchSteps; ++it) {
        if (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (o.stamp[mid] <= fs) lo = mid + 1; else hi = mid;
        }
    }
    const double* src = lo > b ? o.pose + 3 * (size_t)(lo - 1) : o.start + 3 * s;
    const double y = src[1];
    o.frame_pose[3 * (size_t)f] = src[0]; o.frame_pose[3 * (size_t)f + 1] = o.flip_y ? -y : y; o.frame_pose[3 * (size_t)f + 2] = src[2];
    if (o.frame_cmd) o.frame_cmd[f] = lo > b ? o.orig[lo - 1] : -1;
}

static dim3 odo_grid(int n) { return dim3((unsigned)((n + kOdoThreads - 1) / kOdoThreads)); }

void launch_odo_prepare(const OdoStep& o, hipStream_t s) { hipLaunchKernelGGL(k_odo_prepare, odo_grid(o.n_commands), dim3(kOdoThreads), 0, s, o); }
void launch_odo_heading(const OdoStep& o, hipStream_t s) { hipLaunchKernelGGL(k_odo_heading, dim3(o.n_streams), dim3(kOdoChunk), 0, s, o); }
void launch_odo_terms(const OdoStep& o, hipStream_t s) { hipLaunchKernelGGL(k_odo_terms, odo_grid(o.n_commands), dim3(kOdoThreads), 0, s, o); }
void launch_odo_position(const OdoStep& o, hipStream_t s) { hipLaunchKernelGGL(k_odo_position, dim3(o.n_streams), dim3(kOdoChunk), 0, s, o); }
void launch_odo_sample(const OdoStep& o, hipStream_t s) { hipLaunchKernelGGL(k_odo_sample, odo_grid(o.n_frames), dim3(kOdoThreads), 0, s, o); }

}  // namespace lf
