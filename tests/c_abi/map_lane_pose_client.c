/* A plain-C client of include/lanefront.h's lane pose: built with -Werror from the header alone.  Without arguments it prints the
 * sizes of lf_lane_pose_config, lf_map_lane_pose_record and lf_lane_pose_result as this compiler lays them out and as the library
 * reports them, then the default configuration (lf_map_lane_pose_default_config runs on the host and opens no device).
 * With the argument "run" it seeds a map of twelve entries -- a white line of six marks 0.125 m apart along y = 0.03 and a yellow
 * one along y = 0.28 -- and prints what lf_map_lane_pose makes of three poses under the default configuration, then the code and
 * the text of one refused call and the outputs it left alone. */
#include <stdio.h>
#include <string.h>
#include "lanefront.h"

static int run(void)
{
    static const double ground[48] = { 0.0, 0.03, 0.1, 0.03,  0.125, 0.03, 0.225, 0.03,  0.25, 0.03, 0.35, 0.03,  0.375, 0.03, 0.475, 0.03,
                                       0.5, 0.03, 0.6, 0.03,  0.625, 0.03, 0.725, 0.03,
                                       0.0, 0.28, 0.1, 0.28,  0.125, 0.28, 0.225, 0.28,  0.25, 0.28, 0.35, 0.28,  0.375, 0.28, 0.475, 0.28,
                                       0.5, 0.28, 0.6, 0.28,  0.625, 0.28, 0.725, 0.28 };
    static const uint8_t color[12] = { 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1 };
    static const double frame_pose[9] = { 0.3, 0.155, 0.0,  0.4, 0.2, 0.1,  5.0, 5.0, 0.0 };
    uint8_t code[12 * 32];
    lf_map_lane_pose_record p[3];
    lf_lane_pose_config c;
    lf_lane_pose_result res;
    lf_map_config mc;
    lf_map* m = NULL;
    int k, rc;
    memset(code, 0, sizeof(code));
    memset(&mc, 0, sizeof(mc));
    mc.capacity = 64; mc.max_distance = 128;
    if ((rc = lf_map_create(0, &mc, &m)) != LF_OK) { fprintf(stderr, "lf_map_create: %s\n", lf_map_last_error(NULL)); return 3; }
    if ((rc = lf_map_seed(m, code, color, ground, 12, 0)) != LF_OK) { fprintf(stderr, "lf_map_seed: %s\n", lf_map_last_error(m)); return 4; }
    lf_map_lane_pose_default_config(&c);
    if ((rc = lf_map_lane_pose(m, &c, frame_pose, 3, &res, p, 0)) != LF_OK) { fprintf(stderr, "lf_map_lane_pose: %s\n", lf_map_last_error(m)); return 5; }
    printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", res.polylines.size, res.polylines.n_lanes, res.polylines.n_participating, res.polylines.n_vertices,
           res.polylines.n_polylines, res.polylines.n_closed, res.polylines.n_edges, res.polylines.reserved_, res.n_edges[0], res.n_edges[1], res.n_posed,
           res.reserved_);
    for (k = 0; k < 3; ++k)
        printf("%a %a %a %a %a %a %a %a %a %d %d %d %d %d %d\n", p[k].d, p[k].phi, p[k].width, p[k].line_d[0], p[k].line_d[1], p[k].line_phi[0], p[k].line_phi[1],
               p[k].line_dist[0], p[k].line_dist[1], p[k].vertex[0], p[k].vertex[1], p[k].polyline[0], p[k].polyline[1], p[k].status, p[k].in_lane);
    /* refused: touches nothing */
    c.radius = 0.0;
    memset(p, 0x11, sizeof(p));
    memset(&res, 0x22, sizeof(res));
    rc = lf_map_lane_pose(m, &c, frame_pose, 3, &res, p, 0);
    printf("%d %d %d\n", rc, p[0].status == 0x11111111, res.n_posed == 0x22222222);
    printf("%s\n", lf_map_last_error(m));
    lf_map_destroy(m);
    return 0;
}

int main(int argc, char** argv)
{
    lf_lane_pose_config c;
    int (*lane_pose)(lf_map*, const lf_lane_pose_config*, const double*, int, lf_lane_pose_result*, lf_map_lane_pose_record*, int) = lf_map_lane_pose;
    int (*timing)(lf_map*, double*, int32_t*) = lf_map_lane_pose_timing;
    if (!lane_pose || !timing) return 2;
    if (argc > 1 && strcmp(argv[1], "run") == 0) return run();
    printf("%d %d %d %d %d %d\n", (int)sizeof(lf_lane_pose_config), lf_sizeof_lane_pose_config(), (int)sizeof(lf_map_lane_pose_record), lf_sizeof_lane_pose(),
           (int)sizeof(lf_lane_pose_result), lf_sizeof_lane_pose_result());
    memset(&c, 0xFF, sizeof(c));
    lf_map_lane_pose_default_config(&c);
    printf("%a %a %a %d %d %d %d %a %a %d %d\n", c.polylines.lanes.radius, c.polylines.lanes.max_offset, c.polylines.lanes.max_sin, c.polylines.lanes.min_hits,
           c.polylines.lanes.min_entries, c.polylines.lanes.color_mask, c.polylines.lanes.reserved_, c.polylines.cell, c.polylines.max_gap, c.polylines.reach,
           c.polylines.reserved_);
    printf("%a %a %a %a %a %d %d\n", c.radius, c.max_sin, c.white_offset, c.yellow_offset, c.max_d, c.min_vertices, c.sides);
    return 0;
}
