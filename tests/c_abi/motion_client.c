/* A plain-C client of the frame motion (include/lanefront_motion.h), the only header it includes: what a visual-odometry node links
 * against.  Compiled by gcc (C11), no HIP headers: only the C ABI.
 *
 *   motion_client
 *       prints the sizes of the two structs (the compiler's and the library's), the five constants and the default configuration
 *       (the doubles as hex floats)
 *   motion_client run <batch.bin> <n> <n_frames> <gate> <out.bin>
 *       batch.bin: int32 frame_offset[n_frames + 1] | double ground[n][4] | uint8 code[n][32] | uint8 color[n]; host arrays, no keep.
 *       One estimate over the consecutive pairs with gate = gate_refine = <gate> and no prior; writes
 *       lf_motion_result results[n_frames - 1] | int32 cand[n_frames - 1][128][3], then makes one refused call and prints its code,
 *       its message and whether the results were left alone.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lanefront_motion.h"

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
    lf_motion_config c;
    memset(&c, 0xff, sizeof(c));
    lf_motion_default_config(&c);
    if (argc == 1) {
        printf("%zu %zu %d %d %d %d %d %d %d\n", sizeof(lf_motion_config), sizeof(lf_motion_result), lf_sizeof_motion_config(), lf_sizeof_motion_result(),
               LF_MOTION_MAX_FRAMES, LF_MOTION_MAX_CANDIDATES, LF_MOTION_SOURCE_NONE, LF_MOTION_SOURCE_SEARCH, LF_MOTION_SOURCE_PRIOR);
        printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", (int)c.cross_check, (int)c.max_distance, (int)c.min_margin, (int)c.color_match, (int)c.kept_only,
               (int)c.search, (int)c.max_pairs, (int)c.flips, (int)c.min_inliers, (int)c.iterations, (int)c.min_pairs, (int)c.reserved_);
        printf("%a %a %a %a %a %a %a %a\n", c.gate, c.min_sin, c.gate_refine, c.huber, c.prior_xy, c.prior_theta, c.max_shift, c.max_turn);
        return 0;
    }
    if (argc != 7 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: motion_client [run <batch.bin> <n> <n_frames> <gate> <out.bin>]\n"); return 2; }
    const int n = atoi(argv[3]), n_frames = atoi(argv[4]);
    if (n < 1 || n_frames < 2) { fprintf(stderr, "n must be >= 1 and n_frames >= 2\n"); return 2; }
    c.gate = c.gate_refine = atof(argv[5]);
    const size_t fo_bytes = ((size_t)n_frames + 1) * 4, sn = (size_t)n, np = (size_t)n_frames - 1;
    uint8_t* raw = (uint8_t*)xread(argv[2], fo_bytes + sn * (32 + 32 + 1));
    /* (fo_bytes is a multiple of 4, not of 8: the doubles are copied to storage of their own) */
    double* ground = (double*)malloc(sn * 32);
    memcpy(ground, raw + fo_bytes, sn * 32);
    lf_segments s;
    memset(&s, 0, sizeof(s));
    s.capacity = n;
    s.frame_offset = (int32_t*)raw;
    s.ground = ground;
    s.code = raw + fo_bytes + sn * 32;
    s.color = raw + fo_bytes + sn * 64;
    lf_motion* mo = NULL;
    int rc = lf_motion_create(0, (int)np, &mo);
    if (rc) { fprintf(stderr, "lf_motion_create: %d (%s)\n", rc, lf_motion_last_error(NULL)); return 3; }
    lf_motion_result* res = (lf_motion_result*)calloc(np, sizeof(lf_motion_result));
    const size_t cand_count = np * LF_MOTION_MAX_CANDIDATES * 3;
    int32_t* cand = (int32_t*)calloc(cand_count, sizeof(int32_t));
    rc = lf_motion_estimate(mo, NULL, &s, n, n_frames, NULL, (int)np, NULL, &c, 0, res, cand);
    if (rc) { fprintf(stderr, "lf_motion_estimate: %d (%s)\n", rc, lf_motion_last_error(mo)); return 3; }
    FILE* o = fopen(argv[6], "wb");
    if (!o || fwrite(res, sizeof(lf_motion_result), np, o) != np || fwrite(cand, sizeof(int32_t), cand_count, o) != cand_count) { perror(argv[6]); return 2; }
    fclose(o);
    /* one pair too many for the handle is refused, and nothing moves */
    lf_motion_result* again = (lf_motion_result*)malloc(np * sizeof(lf_motion_result));
    memcpy(again, res, np * sizeof(lf_motion_result));
    const int32_t ab[4] = { 0, 1, 1, 0 };
    rc = lf_motion_estimate(mo, NULL, &s, n, n_frames, np == 1 ? ab : NULL, np == 1 ? 2 : (int)np + 1, NULL, &c, 0, again, NULL);
    printf("%d\n%s\n%d\n", rc, lf_motion_last_error(mo), memcmp(res, again, np * sizeof(lf_motion_result)) == 0);
    if (lf_motion_synchronize(mo) != LF_OK) return 3;
    lf_motion_destroy(mo);
    free(res); free(again); free(cand); free(ground); free(raw);
    return 0;
}
