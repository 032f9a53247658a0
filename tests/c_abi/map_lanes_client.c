/* A plain-C client of include/lanefront.h's lane lines: built with -Werror from the header alone.  Without arguments it prints the
 * sizes of lf_lanes_config, lf_lane and lf_lanes_result as this compiler lays them out and as the library reports them, then the
 * default configuration (lf_map_lanes_default_config runs on the host and opens no device).  With the argument "run" it seeds a
 * map of seven entries -- a line of four marks, a line of two, a mark across the first line -- and prints what lf_map_lanes makes
 * of it under the default configuration, then the code and the text of one refused call and the outputs it left alone. */
#include <stdio.h>
#include <string.h>
#include "lanefront.h"

static int run(void)
{
    static const double ground[28] = { 0.0, 0.0, 0.1, 0.0,  0.125, 0.0, 0.225, 0.0,  0.25, 0.0, 0.35, 0.0,  0.375, 0.0, 0.475, 0.0,
                                       0.0, 2.0, 0.1, 2.0,  0.125, 2.0, 0.225, 2.0,  0.175, -0.05, 0.175, 0.05 };
    static const uint8_t color[7] = { 1, 1, 1, 1, 1, 1, 1 };
    uint8_t code[7 * 32];
    int32_t lane_of[64], n_links[64], support[64];
    lf_lane lanes[4];
    lf_lanes_config c;
    lf_lanes_result res;
    lf_map_config mc;
    lf_map* m = NULL;
    int k, rc;
    memset(code, 0, sizeof(code));
    memset(&mc, 0, sizeof(mc));
    mc.capacity = 64; mc.max_distance = 128;
    if ((rc = lf_map_create(0, &mc, &m)) != LF_OK) { fprintf(stderr, "lf_map_create: %s\n", lf_map_last_error(NULL)); return 3; }
    if ((rc = lf_map_seed(m, code, color, ground, 7, 0)) != LF_OK) { fprintf(stderr, "lf_map_seed: %s\n", lf_map_last_error(m)); return 4; }
    lf_map_lanes_default_config(&c);
    if ((rc = lf_map_lanes(m, &c, &res, lane_of, n_links, support, lanes, 4, 0)) != LF_OK) { fprintf(stderr, "lf_map_lanes: %s\n", lf_map_last_error(m)); return 5; }
    printf("%d %d %d %d %lld\n", res.size, res.n_eligible, res.n_components, res.n_lanes, (long long)res.n_links);
    for (k = 0; k < 8; ++k) printf("%d %d %d\n", lane_of[k], n_links[k], support[k]);
    for (k = 0; k < res.n_lanes; ++k)
        printf("%d %d %d %lld %a %a %a %a\n", lanes[k].first_row, lanes[k].color, lanes[k].n_entries, (long long)lanes[k].hits, lanes[k].box[0], lanes[k].box[1],
               lanes[k].box[2], lanes[k].box[3]);
    /* refused: touches nothing */
    c.radius = 0.0;
    memset(lane_of, 0x11, sizeof(lane_of));
    memset(&res, 0x22, sizeof(res));
    rc = lf_map_lanes(m, &c, &res, lane_of, NULL, NULL, NULL, 0, 0);
    printf("%d %d %d\n", rc, lane_of[0] == 0x11111111, res.n_lanes == 0x22222222);
    printf("%s\n", lf_map_last_error(m));
    lf_map_destroy(m);
    return 0;
}

int main(int argc, char** argv)
{
    lf_lanes_config c;
    int (*lanes)(lf_map*, const lf_lanes_config*, lf_lanes_result*, int32_t*, int32_t*, int32_t*, lf_lane*, int, int) = lf_map_lanes;
    int (*timing)(lf_map*, double*, int32_t*) = lf_map_lanes_timing;
    if (!lanes || !timing) return 2;
    if (argc > 1 && strcmp(argv[1], "run") == 0) return run();
    printf("%d %d %d %d %d %d\n", (int)sizeof(lf_lanes_config), lf_sizeof_lanes_config(), (int)sizeof(lf_lane), lf_sizeof_lane(),
           (int)sizeof(lf_lanes_result), lf_sizeof_lanes_result());
    memset(&c, 0xFF, sizeof(c));
    lf_map_lanes_default_config(&c);
    printf("%a %a %a %d %d %d %d\n", c.radius, c.max_offset, c.max_sin, c.min_hits, c.min_entries, c.color_mask, c.reserved_);
    return 0;
}
