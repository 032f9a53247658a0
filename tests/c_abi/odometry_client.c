/* A plain-C client of the odometry (include/lanefront_odometry.h), the only header it includes: what a node's integrator links
 * against.  Compiled by gcc (C11), no HIP headers: only the C ABI.
 *
 *   odometry_client
 *       prints the sizes of the two structs, the three constants and the default configuration (the doubles as hex floats)
 *   odometry_client run <commands.bin> <n> <start.bin> <poses.bin>
 *       commands.bin: int64 stamp_ns[n] | double vel_left[n] | double vel_right[n]; start.bin: double x, y, theta, last_t.
 *       One stream from that state, one step over the commands with a frame at every command's stamp; writes
 *       double trajectory[n][3] | double frame_pose[n][3] | int32 frame_cmd[n] | uint8 driven[n], prints the final state, then makes
 *       one refused call and prints its code, its message and the counters again.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lanefront_odometry.h"

static void* xread(const char* path, size_t bytes)
{
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    void* p = malloc(bytes ? bytes : 1);
    if (fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "%s: short read\n", path); exit(2); }
    fclose(f);
    return p;
}

int main(int argc, char** argv)
{
    lf_odometry_config c;
    memset(&c, 0xff, sizeof(c));
    lf_odometry_default_config(&c);
    if (argc == 1) {
        printf("%zu %zu %d %d %d\n", sizeof(lf_odometry_config), sizeof(lf_odometry_state), LF_ODOMETRY_STAMP_NSECS, LF_ODOMETRY_STAMP_FULL, LF_ODOMETRY_MAX_STREAMS);
        printf("%a %a %d %d\n", c.wheel_distance, c.dt_max, (int)c.stamp_mode, (int)c.flip_y);
        return 0;
    }
    if (argc != 6 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: odometry_client [run <commands.bin> <n> <start.bin> <poses.bin>]\n"); return 2; }
    const int n = atoi(argv[3]);
    if (n < 1) { fprintf(stderr, "n must be >= 1\n"); return 2; }
    uint8_t* cmds = (uint8_t*)xread(argv[2], (size_t)n * 24);
    const int64_t* stamp = (const int64_t*)cmds;
    const double *vl = (const double*)(cmds + (size_t)n * 8), *vr = (const double*)(cmds + (size_t)n * 16);
    double* start = (double*)xread(argv[4], 4 * sizeof(double));
    lf_odometry* od = NULL;
    int rc = lf_odometry_create(0, &c, 1, n, n, &od);
    if (rc) { fprintf(stderr, "lf_odometry_create: %d (%s)\n", rc, lf_odometry_last_error(NULL)); return 3; }
    lf_odometry_state st;
    memset(&st, 0, sizeof(st));
    st.x = start[0]; st.y = start[1]; st.theta = start[2]; st.last_t = start[3];
    rc = lf_odometry_reset(od, 0, &st);
    if (rc) { fprintf(stderr, "lf_odometry_reset: %d (%s)\n", rc, lf_odometry_last_error(od)); return 3; }
    double* traj = (double*)calloc((size_t)n * 3, sizeof(double));
    double* pose = (double*)calloc((size_t)n * 3, sizeof(double));
    int32_t* fcmd = (int32_t*)calloc((size_t)n, sizeof(int32_t));
    uint8_t* driven = (uint8_t*)calloc((size_t)n, 1);
    rc = lf_odometry_step(od, n, stamp, vl, vr, NULL, n, stamp, NULL, pose, fcmd, traj, driven, 0);
    if (rc) { fprintf(stderr, "lf_odometry_step: %d (%s)\n", rc, lf_odometry_last_error(od)); return 3; }
    FILE* o = fopen(argv[5], "wb");
    if (!o || fwrite(traj, 24, (size_t)n, o) != (size_t)n || fwrite(pose, 24, (size_t)n, o) != (size_t)n || fwrite(fcmd, 4, (size_t)n, o) != (size_t)n ||
        fwrite(driven, 1, (size_t)n, o) != (size_t)n) { perror(argv[5]); return 2; }
    fclose(o);
    rc = lf_odometry_get_state(od, 0, &st);
    if (rc) { fprintf(stderr, "lf_odometry_get_state: %d (%s)\n", rc, lf_odometry_last_error(od)); return 3; }
    printf("%a %a %a %a %lld %lld %lld\n", st.x, st.y, st.theta, st.last_t, (long long)st.last_stamp_ns, (long long)st.n_commands, (long long)st.n_driven);
    /* a stamp below where the stream stands is refused, and nothing moves */
    const int64_t early = stamp[n - 1] - 1;
    const double v = 0.5;
    rc = lf_odometry_step(od, 1, &early, &v, &v, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, 0);
    printf("%d\n%s\n", rc, lf_odometry_last_error(od));
    lf_odometry_state again;
    if (lf_odometry_get_state(od, 0, &again) != LF_OK) return 3;
    printf("%d\n", memcmp(&st, &again, sizeof(st)) == 0);
    lf_odometry_destroy(od);
    free(traj); free(pose); free(fcmd); free(driven); free(cmds); free(start);
    return 0;
}
