/* A plain-C client of include/lanefront.h's map pruning: built with -Werror from the header alone.  Without arguments it prints the
 * sizes of lf_prune_config and lf_prune_result as this compiler lays them out and as the library reports them, then the default
 * configuration (lf_map_prune_default_config runs on the host and opens no device).  With the argument "run" it seeds a map of six
 * entries, prunes it with the cover rule and prints the result, the remap and the survivors' ground. */
#include <stdio.h>
#include <string.h>
#include "lanefront.h"

static int run(void)
{
    /* three copies of one line, a shorter one inside it, one far away, one of another colour on top of the first */
    static const double ground[24] = { 0.0, 0.0, 4.0, 0.0,  0.0, 0.0, 4.0, 0.0,  1.0, 0.0, 2.0, 0.0,  0.0, 9.0, 4.0, 9.0,  0.0, 0.0, 4.0, 0.0,  0.0, 0.0, 4.0, 0.0 };
    static const uint8_t color[6] = { 0, 0, 0, 0, 0, 1 };
    uint8_t code[6 * 32];
    double got[6 * 4];
    int32_t remap[64];
    lf_map_config mc;
    lf_map* m = NULL;
    lf_prune_config c;
    lf_prune_result res;
    int k, rc, size = -1, head = -1;
    for (k = 0; k < 6 * 32; ++k) code[k] = (uint8_t)(k * 37 + 11);
    memset(&mc, 0, sizeof(mc));
    mc.capacity = 64; mc.max_distance = 128;
    if ((rc = lf_map_create(0, &mc, &m)) != LF_OK) { fprintf(stderr, "lf_map_create: %s\n", lf_map_last_error(NULL)); return 3; }
    if ((rc = lf_map_seed(m, code, color, ground, 6, 0)) != LF_OK) { fprintf(stderr, "lf_map_seed: %s\n", lf_map_last_error(m)); return 4; }
    lf_map_prune_default_config(&c);
    c.keep_seeded = 0; c.cover_distance = 0.02;
    if ((rc = lf_map_prune(m, &c, &res, remap, 0)) != LF_OK) { fprintf(stderr, "lf_map_prune: %s\n", lf_map_last_error(m)); return 5; }
    if ((rc = lf_map_size(m, &size, &head, NULL, NULL)) != LF_OK) return 6;
    printf("%d %d %d %d %d %d %d %d\n", res.size_before, res.size_after, res.n_stale, res.n_weak, res.n_box, res.n_covered, size, head);
    for (k = 0; k < 8; ++k) printf("%d ", remap[k]);
    printf("\n");
    if (res.size_after < 0 || res.size_after > 6) return 7;
    if ((rc = lf_map_fetch(m, 0, res.size_after, NULL, NULL, got, NULL, NULL)) != LF_OK) return 8;
    for (k = 0; k < 4 * res.size_after; ++k) printf("%a ", got[k]);
    printf("\n");
    lf_map_destroy(m);
    return 0;
}

int main(int argc, char** argv)
{
    lf_prune_config c;
    int (*prune)(lf_map*, const lf_prune_config*, lf_prune_result*, int32_t*, int) = lf_map_prune;
    int (*timing)(lf_map*, double*, int32_t*) = lf_map_prune_timing;
    if (!prune || !timing) return 2;
    if (argc > 1 && strcmp(argv[1], "run") == 0) return run();
    printf("%d %d %d %d\n", (int)sizeof(lf_prune_config), lf_sizeof_prune_config(), (int)sizeof(lf_prune_result), lf_sizeof_prune_result());
    memset(&c, 0xFF, sizeof(c));
    lf_map_prune_default_config(&c);
    printf("%d %d %d %d %d %d %d %d\n", c.min_hits, c.weak_before, c.stale_before, c.keep_seeded, c.color_mask, c.use_box, c.cover_max_entries, c.reserved_);
    printf("%a %a %a %a %a %a\n", c.box[0], c.box[1], c.box[2], c.box[3], c.cover_distance, c.cover_slack);
    return 0;
}
