/* A plain-C client of include/lanefront.h's trajectory smoother: built with -Werror from the header alone.  Without arguments it
 * prints the size of lf_smooth_config as this compiler lays it out and as the library reports it, then the default configuration
 * (lf_map_smooth_default_config runs on the host and opens no device).  With the argument "run" it seeds a map of four entries,
 * smooths two chains (two frames, one frame) with host arrays and prints every result in hexadecimal floats. */
#include <stdio.h>
#include <string.h>
#include "lanefront.h"

static int run(void)
{
    /* two lines along x, two across them; three frames that see all four from poses near the origin */
    static const double map_ground[16] = { 0.5, -0.2, 1.5, -0.2, 0.5, 0.3, 1.5, 0.3, 0.8, -0.2, 0.8, 0.3, 1.2, -0.2, 1.2, 0.3 };
    static const uint8_t map_color[4] = { 0, 0, 0, 0 };
    uint8_t map_code[4 * 32], color[12], keep[12];
    double ground[12 * 4];
    const double shift[3] = { 0.01, 0.02, -0.015 };
    const double pose[9] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    const int32_t frame_offset[4] = { 0, 4, 8, 12 }, chain_offset[3] = { 0, 2, 3 };
    int32_t idx[12], chain_status[2];
    float dist[12];
    lf_map_config mc;
    lf_map* m = NULL;
    lf_segments s;
    lf_smooth_config c;
    lf_align_result res[3];
    int f, k, rc;
    for (k = 0; k < 4 * 32; ++k) map_code[k] = (uint8_t)(k * 37 + 11);
    for (f = 0; f < 3; ++f)
        for (k = 0; k < 4; ++k) {
            int e;
            for (e = 0; e < 4; ++e) ground[(4 * f + k) * 4 + e] = map_ground[4 * k + e] - ((e & 1) ? shift[f] : 2.0 * shift[f]);
            idx[4 * f + k] = k; dist[4 * f + k] = 0.0f; color[4 * f + k] = 0; keep[4 * f + k] = 1;
        }
    memset(&mc, 0, sizeof(mc));
    mc.capacity = 64; mc.max_distance = 128;
    if ((rc = lf_map_create(0, &mc, &m)) != LF_OK) { fprintf(stderr, "lf_map_create: %s\n", lf_map_last_error(NULL)); return 3; }
    if ((rc = lf_map_seed(m, map_code, map_color, map_ground, 4, 0)) != LF_OK) { fprintf(stderr, "lf_map_seed: %s\n", lf_map_last_error(m)); return 4; }
    memset(&s, 0, sizeof(s));
    s.capacity = 12; s.frame_offset = (int32_t*)frame_offset; s.ground = ground; s.color = color; s.keep = keep;
    lf_map_smooth_default_config(&c);
    c.align.min_pairs = 2;
    rc = lf_map_smooth(m, NULL, &s, 12, 3, idx, dist, pose, chain_offset, 2, &c, 0, res, chain_status);
    if (rc != LF_OK) { fprintf(stderr, "lf_map_smooth: %s\n", lf_map_last_error(m)); return 5; }
    for (f = 0; f < 3; ++f)
        printf("%a %a %a %a %a %d %d %d %d\n", res[f].x, res[f].y, res[f].theta, res[f].cost0, res[f].cost, res[f].n_pairs, res[f].n_used,
               res[f].iterations, res[f].status);
    printf("%d %d\n", chain_status[0], chain_status[1]);
    lf_map_destroy(m);
    return 0;
}

int main(int argc, char** argv)
{
    lf_smooth_config c;
    int (*smooth)(lf_map*, lf_handle*, const lf_segments*, int, int, const int32_t*, const float*, const double*, const int32_t*, int,
                  const lf_smooth_config*, int, lf_align_result*, int32_t*) = lf_map_smooth;
    int (*step)(lf_map*, lf_handle*, const lf_segments*, int, int, const double*, const int32_t*, int, const lf_smooth_config*, int, int32_t*,
                float*, lf_align_result*, int32_t*) = lf_map_step_smoothed;
    int (*step_host)(lf_map*, const lf_segments*, int, int, const double*, const int32_t*, int, const lf_smooth_config*, int, int32_t*, float*,
                     lf_align_result*, int32_t*) = lf_map_step_smoothed_host;
    int (*timing)(lf_map*, double*, int32_t*) = lf_map_smooth_timing;
    if (!smooth || !step || !step_host || !timing) return 2;
    if (argc > 1 && strcmp(argv[1], "run") == 0) return run();
    printf("%d %d %d\n", (int)sizeof(lf_smooth_config), lf_sizeof_smooth_config(), lf_sizeof_align_config());
    lf_map_smooth_default_config(&c);
    printf("%d %d %d %d\n", c.align.iterations, c.align.min_pairs, c.align.min_hits, c.align.color_match);
    printf("%a %f %f %a %a %f %f\n", c.align.gate, c.align.huber, c.align.max_dist, c.align.prior_xy, c.align.prior_theta, c.align.max_shift,
           c.align.max_turn);
    printf("%a %a %a %a\n", c.odo_xy, c.odo_theta, c.anchor_xy, c.anchor_theta);
    return 0;
}
