/* A plain-C client of include/lanefront.h's polylines: built with -Werror from the header alone.  Without arguments it prints the
 * sizes of lf_polylines_config, lf_polyline_vertex, lf_polyline and lf_polylines_result as this compiler lays them out and as the
 * library reports them, then the default configuration (lf_map_polylines_default_config runs on the host and opens no device).
 * With the argument "run" it seeds a map of eight entries -- a line of six marks 0.125 m apart and two marks far away -- and prints
 * what lf_map_polylines makes of it under the default configuration, then the code and the text of one refused call and the
 * outputs it left alone. */
#include <stdio.h>
#include <string.h>
#include "lanefront.h"

static int run(void)
{
    static const double ground[32] = { 0.0, 0.03, 0.1, 0.03,  0.125, 0.03, 0.225, 0.03,  0.25, 0.03, 0.35, 0.03,  0.375, 0.03, 0.475, 0.03,
                                       0.5, 0.03, 0.6, 0.03,  0.625, 0.03, 0.725, 0.03,  0.0, 2.0, 0.1, 2.0,  0.125, 2.0, 0.225, 2.0 };
    static const uint8_t color[8] = { 1, 1, 1, 1, 1, 1, 1, 1 };
    uint8_t code[8 * 32];
    int32_t vertex_of[64];
    lf_polyline_vertex v[8];
    lf_polyline p[4];
    lf_polylines_config c;
    lf_polylines_result res;
    lf_map_config mc;
    lf_map* m = NULL;
    int k, rc;
    memset(code, 0, sizeof(code));
    memset(&mc, 0, sizeof(mc));
    mc.capacity = 64; mc.max_distance = 128;
    if ((rc = lf_map_create(0, &mc, &m)) != LF_OK) { fprintf(stderr, "lf_map_create: %s\n", lf_map_last_error(NULL)); return 3; }
    if ((rc = lf_map_seed(m, code, color, ground, 8, 0)) != LF_OK) { fprintf(stderr, "lf_map_seed: %s\n", lf_map_last_error(m)); return 4; }
    lf_map_polylines_default_config(&c);
    if ((rc = lf_map_polylines(m, &c, &res, vertex_of, v, 8, p, 4, 0)) != LF_OK) { fprintf(stderr, "lf_map_polylines: %s\n", lf_map_last_error(m)); return 5; }
    printf("%d %d %d %d %d %d %d %d\n", res.size, res.n_lanes, res.n_participating, res.n_vertices, res.n_polylines, res.n_closed, res.n_edges, res.reserved_);
    for (k = 0; k < 9; ++k) printf("%d ", vertex_of[k]);
    printf("\n%d %d\n", res.n_vertices, res.n_polylines);
    for (k = 0; k < res.n_vertices; ++k)
        printf("%d %d %d %d %d %d %lld %a %a %a %a\n", v[k].lane, v[k].first_row, v[k].n_entries, v[k].polyline, v[k].cx, v[k].cy, (long long)v[k].hits, v[k].x,
               v[k].y, v[k].tx, v[k].ty);
    for (k = 0; k < res.n_polylines; ++k)
        printf("%d %d %d %d %d %d %lld\n", p[k].lane, p[k].first_vertex, p[k].n_vertices, p[k].closed, p[k].first_row, p[k].n_entries, (long long)p[k].hits);
    /* refused: touches nothing */
    c.cell = 0.0;
    memset(vertex_of, 0x11, sizeof(vertex_of));
    memset(&res, 0x22, sizeof(res));
    rc = lf_map_polylines(m, &c, &res, vertex_of, NULL, 0, NULL, 0, 0);
    printf("%d %d %d\n", rc, vertex_of[0] == 0x11111111, res.n_vertices == 0x22222222);
    printf("%s\n", lf_map_last_error(m));
    lf_map_destroy(m);
    return 0;
}

int main(int argc, char** argv)
{
    lf_polylines_config c;
    int (*polylines)(lf_map*, const lf_polylines_config*, lf_polylines_result*, int32_t*, lf_polyline_vertex*, int, lf_polyline*, int, int) = lf_map_polylines;
    int (*timing)(lf_map*, double*, int32_t*) = lf_map_polylines_timing;
    if (!polylines || !timing) return 2;
    if (argc > 1 && strcmp(argv[1], "run") == 0) return run();
    printf("%d %d %d %d %d %d %d %d\n", (int)sizeof(lf_polylines_config), lf_sizeof_polylines_config(), (int)sizeof(lf_polyline_vertex),
           lf_sizeof_polyline_vertex(), (int)sizeof(lf_polyline), lf_sizeof_polyline(), (int)sizeof(lf_polylines_result), lf_sizeof_polylines_result());
    memset(&c, 0xFF, sizeof(c));
    lf_map_polylines_default_config(&c);
    printf("%a %a %a %d %d %d %d %a %a %d %d\n", c.lanes.radius, c.lanes.max_offset, c.lanes.max_sin, c.lanes.min_hits, c.lanes.min_entries, c.lanes.color_mask,
           c.lanes.reserved_, c.cell, c.max_gap, c.reach, c.reserved_);
    return 0;
}
