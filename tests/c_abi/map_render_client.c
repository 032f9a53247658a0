/* A plain-C client of the live map's top-down view (include/lanefront.h "lf_map_render"): seeds a map with a few hand-placed
 * entries, renders lf_map_default_view to the host and prints the counts and the 64-bit FNV-1a hash of the image.
 *
 *   map_render_client            prints "<n_drawn> <n_skipped> <hash as 16 hex digits>"
 *
 * Compiled by gcc (C11), no HIP headers: only the C ABI.  tests/test_c_abi_map_render.py holds the same entries.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lanefront.h"

#define N 6

int main(void)
{
    static const double ground[N][4] = { { -3.0, -2.0, 4.0, 1.5 }, { 0.25, 7.0, 0.5, -7.0 }, { -8.0, 8.0, 8.0, -8.0 },
                                         { 2.0, 2.0, 2.0, 2.0 }, { -100.0, 3.0, 100.0, 3.5 }, { 1.0, 1.0, 1e300, 1.0 } };
    static const uint8_t color[N] = { 0, 1, 2, 0, 1, 7 };
    static const double trajectory[3][2] = { { -6.0, -6.0 }, { 0.0, -5.0 }, { 6.0, 6.0 } };
    uint8_t code[N][32];
    for (int i = 0; i < N; ++i) memset(code[i], 17 * (i + 1), 32);
    lf_map_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.capacity = 64; cfg.max_distance = 128; cfg.policy = LF_MAP_APPEND; cfg.when_full = LF_MAP_RING;
    lf_map* m = NULL;
    int rc = lf_map_create(0, &cfg, &m);
    if (rc) { fprintf(stderr, "lf_map_create: %d (%s)\n", rc, lf_map_last_error(NULL)); return 3; }
    if ((rc = lf_map_seed(m, &code[0][0], color, &ground[0][0], N, 0))) { fprintf(stderr, "lf_map_seed: %d (%s)\n", rc, lf_map_last_error(m)); return 4; }
    lf_map_view v;
    lf_map_default_view(&v);
    uint8_t* img = (uint8_t*)malloc((size_t)v.rows * v.cols * 3);
    int n_drawn = -1, n_skipped = -1, again_drawn = -1, again_skipped = -1;
    rc = lf_map_render(m, &v, &trajectory[0][0], 3, img, 0, &n_drawn, &n_skipped);
    if (rc) { fprintf(stderr, "lf_map_render: %d (%s)\n", rc, lf_map_last_error(m)); return 5; }
    if (lf_map_render_counts(m, &again_drawn, &again_skipped) || again_drawn != n_drawn || again_skipped != n_skipped) { fprintf(stderr, "lf_map_render_counts\n"); return 6; }
    double box[4];
    int n_entries = 0;
    if (lf_map_bounds(m, NULL, box, &n_entries) || n_entries != N || box[0] != -100.0 || box[3] != 8.0) { fprintf(stderr, "lf_map_bounds\n"); return 7; }
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < (size_t)v.rows * v.cols * 3; ++i) h = (h ^ img[i]) * 0x100000001b3ull;
    printf("%d %d %016llx\n", n_drawn, n_skipped, (unsigned long long)h);
    free(img);
    lf_map_destroy(m);
    return 0;
}
