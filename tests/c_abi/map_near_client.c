/* A plain-C client of include/lanefront.h's gated association: built with -Werror from the header alone.  Without arguments it
 * prints the size of lf_near_config as this compiler lays it out and as the library reports it, then the default configuration
 * (lf_map_near_default_config runs on the host and opens no device).  With the argument "run" it seeds a map of four entries,
 * associates three segments of one frame through a pose and prints idx, dist and n_near, then what lf_map_get_near says before and
 * after lf_map_set_near. */
#include <stdio.h>
#include <string.h>
#include "lanefront.h"

static int run(void)
{
    /* two copies of one line, a parallel line 0.05 m above it, a line far away */
    static const double ground[16] = { 0.0, 0.0, 1.0, 0.0,  0.0, 0.0, 1.0, 0.0,  0.0, 0.0625, 1.0, 0.0625,  0.0, 9.0, 1.0, 9.0 };
    static const uint8_t color[4] = { 0, 0, 0, 0 };
    /* the frame's pose moves the segments by (2, 1): on the lines, 0.03 m above them (nearer to the parallel one), far from all */
    static double seg_ground[12] = { -1.75, -1.0, -1.25, -1.0,  -1.75, -0.96875, -1.25, -0.96875,  -1.75, 3.0, -1.25, 3.0 };
    static const double pose[3] = { 2.0, 1.0, 0.0 };
    static int32_t frame_offset[2] = { 0, 3 };
    uint8_t code[4 * 32], seg_code[3 * 32];
    int32_t idx[3], n_near[3];
    float dist[3];
    lf_map_config mc;
    lf_map* m = NULL;
    lf_near_config c, got;
    lf_segments s;
    int k, rc, before, after;
    memset(code, 0, sizeof(code));
    memset(seg_code, 0, sizeof(seg_code));
    code[2 * 32] = 0x07;                 /* the parallel line is 3 bits away from the segments */
    memset(&mc, 0, sizeof(mc));
    mc.capacity = 64; mc.max_distance = 128;
    if ((rc = lf_map_create(0, &mc, &m)) != LF_OK) { fprintf(stderr, "lf_map_create: %s\n", lf_map_last_error(NULL)); return 3; }
    if ((rc = lf_map_seed(m, code, color, ground, 4, 0)) != LF_OK) { fprintf(stderr, "lf_map_seed: %s\n", lf_map_last_error(m)); return 4; }
    memset(&s, 0, sizeof(s));
    s.capacity = 3; s.frame_offset = frame_offset; s.code = seg_code; s.ground = seg_ground;
    lf_map_near_default_config(&c);
    if ((rc = lf_map_associate_near(m, NULL, &s, 3, 1, pose, &c, idx, dist, n_near, 0)) != LF_OK) { fprintf(stderr, "lf_map_associate_near: %s\n", lf_map_last_error(m)); return 5; }
    for (k = 0; k < 3; ++k) printf("%d %g %d\n", idx[k], (double)dist[k], n_near[k]);
    before = lf_map_get_near(m, &got);
    c.radius = 0.5;
    if ((rc = lf_map_set_near(m, &c)) != LF_OK) return 6;
    memset(&got, 0, sizeof(got));
    after = lf_map_get_near(m, &got);
    printf("%d %d %a\n", before, after, got.radius);
    if ((rc = lf_map_set_near(m, NULL)) != LF_OK) return 7;
    printf("%d\n", lf_map_get_near(m, &got));
    lf_map_destroy(m);
    return 0;
}

int main(int argc, char** argv)
{
    lf_near_config c;
    int (*near)(lf_map*, lf_handle*, const lf_segments*, int, int, const double*, const lf_near_config*, int32_t*, float*, int32_t*, int) = lf_map_associate_near;
    int (*timing)(lf_map*, double*, int32_t*) = lf_map_near_timing;
    if (!near || !timing) return 2;
    if (argc > 1 && strcmp(argv[1], "run") == 0) return run();
    printf("%d %d\n", (int)sizeof(lf_near_config), lf_sizeof_near_config());
    memset(&c, 0xFF, sizeof(c));
    lf_map_near_default_config(&c);
    printf("%a %a %a %d %d\n", c.radius, c.max_offset, c.max_sin, c.min_hits, c.reserved_);
    return 0;
}
