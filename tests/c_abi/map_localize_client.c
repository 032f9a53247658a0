/* A plain-C client of include/lanefront.h's localisation against the live map: built with -Werror from the header alone.  Without
 * arguments it prints the sizes of lf_localize_config and lf_localize_result as this compiler lays them out and as the library
 * reports them, then the default configuration (lf_map_localize_default_config runs on the host and opens no device).  With the
 * argument "run" it seeds a map of four entries, localises three frames with host arrays and prints every result in hexadecimal
 * floats. */
#include <stdio.h>
#include <string.h>
#include "lanefront.h"

static int run(void)
{
    /* two lines along x, two across them; frames 0 and 1 see all four from poses shifted by (2 s, s), frame 2 sees one */
    static const double map_ground[16] = { 0.5, -0.2, 1.5, -0.2, 0.5, 0.3, 1.5, 0.3, 0.8, -0.2, 0.8, 0.3, 1.2, -0.2, 1.2, 0.3 };
    static const uint8_t map_color[4] = { 0, 0, 0, 0 };
    uint8_t map_code[4 * 32], color[9], keep[9];
    double ground[9 * 4];
    const double shift[3] = { 2.5, -4.0, 1.0 };
    const double fallback[9] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 7.0, 8.0, 9.0 };
    const int32_t frame_offset[4] = { 0, 4, 8, 9 };
    int32_t idx[9];
    float dist[9];
    lf_map_config mc;
    lf_map* m = NULL;
    lf_segments s;
    lf_localize_config c;
    lf_localize_result res[3];
    int f, k, rc;
    for (k = 0; k < 4 * 32; ++k) map_code[k] = (uint8_t)(k * 37 + 11);
    for (k = 0; k < 9; ++k) {
        int e;
        f = k / 4;
        for (e = 0; e < 4; ++e) ground[k * 4 + e] = map_ground[4 * (k % 4) + e] - ((e & 1) ? shift[f] : 2.0 * shift[f]);
        idx[k] = k % 4; dist[k] = 0.0f; color[k] = 0; keep[k] = 1;
    }
    memset(&mc, 0, sizeof(mc));
    mc.capacity = 64; mc.max_distance = 128;
    if ((rc = lf_map_create(0, &mc, &m)) != LF_OK) { fprintf(stderr, "lf_map_create: %s\n", lf_map_last_error(NULL)); return 3; }
    if ((rc = lf_map_seed(m, map_code, map_color, map_ground, 4, 0)) != LF_OK) { fprintf(stderr, "lf_map_seed: %s\n", lf_map_last_error(m)); return 4; }
    memset(&s, 0, sizeof(s));
    s.capacity = 9; s.frame_offset = (int32_t*)frame_offset; s.ground = ground; s.color = color; s.keep = keep;
    lf_map_localize_default_config(&c);
    rc = lf_map_localize(m, NULL, &s, 9, 3, idx, dist, fallback, &c, 0, res);
    if (rc != LF_OK) { fprintf(stderr, "lf_map_localize: %s\n", lf_map_last_error(m)); return 5; }
    for (f = 0; f < 3; ++f)
        printf("%a %a %a %a %d %d %d %d %d %d %d %d\n", res[f].x, res[f].y, res[f].theta, res[f].cost, res[f].n_pairs, res[f].n_candidates,
               res[f].n_hypotheses, res[f].n_inliers, res[f].seg_a, res[f].seg_b, res[f].flip, res[f].status);
    lf_map_destroy(m);
    return 0;
}

int main(int argc, char** argv)
{
    lf_localize_config c;
    int (*localize)(lf_map*, lf_handle*, const lf_segments*, int, int, const int32_t*, const float*, const double*, const lf_localize_config*,
                    int, lf_localize_result*) = lf_map_localize;
    int (*timing)(lf_map*, double*, int32_t*) = lf_map_localize_timing;
    if (!localize || !timing) return 2;
    if (argc > 1 && strcmp(argv[1], "run") == 0) return run();
    printf("%d %d %d %d\n", (int)sizeof(lf_localize_config), lf_sizeof_localize_config(), (int)sizeof(lf_localize_result),
           lf_sizeof_localize_result());
    lf_map_localize_default_config(&c);
    printf("%d %d %d %d %d %d\n", c.max_pairs, c.flips, c.min_inliers, c.min_hits, c.color_match, c.reserved_);
    printf("%a %a %f\n", c.gate, c.min_sin, c.max_dist);
    return 0;
}
