/* A plain-C client of the key-frame store (include/lanefront_places.h), the only header it includes: what a loop-closure node links
 * against.  Compiled by gcc (C11), no HIP headers: only the C ABI.
 *
 *   places_client
 *       prints the sizes of the two structs (the compiler's and the library's), the five constants and the default configuration
 *   places_client run <batch.bin> <n> <n_frames> <n_keys> <out.bin>
 *       batch.bin: int32 frame_offset[n_frames + 1] | double ground[n][4] | uint8 code[n][32] | uint8 color[n]; host arrays, no keep.
 *       Frames 0 .. n_keys - 1 become keys; every frame is queried with the default configuration; frame n_frames - 1 is measured
 *       against key 0 with the motion's default configuration.  Writes lf_place_hit hits[n_frames][4] | int32 scores[n_frames][n_keys] |
 *       lf_motion_result result, then makes one refused call and prints its code, its message and whether the hits were left alone.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lanefront_places.h"

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
    lf_places_config c;
    memset(&c, 0xff, sizeof(c));
    lf_places_default_config(&c);
    if (argc == 1) {
        printf("%zu %zu %d %d %d %d %d %d %d\n", sizeof(lf_places_config), sizeof(lf_place_hit), lf_sizeof_places_config(), lf_sizeof_place_hit(),
               LF_PLACES_MAX_KEYS, LF_PLACES_MAX_SEGMENTS, LF_PLACES_MAX_QUERIES, LF_PLACES_MAX_SCORES, LF_PLACES_MAX_TOP_K);
        printf("%d %d %d %d %d %d %d %d\n", (int)c.cross_check, (int)c.max_distance, (int)c.min_margin, (int)c.color_match, (int)c.kept_only, (int)c.top_k,
               (int)c.min_score, (int)c.key_gap);
        return 0;
    }
    if (argc != 7 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: places_client [run <batch.bin> <n> <n_frames> <n_keys> <out.bin>]\n"); return 2; }
    const int n = atoi(argv[3]), n_frames = atoi(argv[4]), n_keys = atoi(argv[5]);
    if (n < 1 || n_frames < 1 || n_keys < 1 || n_keys > n_frames) { fprintf(stderr, "n, n_frames >= 1 and 1 <= n_keys <= n_frames\n"); return 2; }
    const size_t fo_bytes = ((size_t)n_frames + 1) * 4, sn = (size_t)n, nf = (size_t)n_frames, nk = (size_t)n_keys;
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
    lf_places* pl = NULL;
    int rc = lf_places_create(0, n_keys, n, n_frames, &pl);
    if (rc) { fprintf(stderr, "lf_places_create: %d (%s)\n", rc, lf_places_last_error(NULL)); return 3; }
    int32_t* frames = (int32_t*)malloc(nk * sizeof(int32_t));
    for (int k = 0; k < n_keys; ++k) frames[k] = k;
    int32_t first = -1, count = -1, stored = -1;
    rc = lf_places_add(pl, NULL, &s, n, n_frames, frames, n_keys, 0, &first);
    if (rc || first != 0 || lf_places_count(pl, &count, &stored) != LF_OK || count != n_keys) { fprintf(stderr, "lf_places_add: %d (%s)\n", rc, lf_places_last_error(pl)); return 3; }
    lf_place_hit* hits = (lf_place_hit*)calloc(nf * (size_t)c.top_k, sizeof(lf_place_hit));
    int32_t* scores = (int32_t*)calloc(nf * nk, sizeof(int32_t));
    rc = lf_places_query(pl, NULL, &s, n, n_frames, NULL, n_frames, NULL, &c, 0, hits, scores);
    if (rc) { fprintf(stderr, "lf_places_query: %d (%s)\n", rc, lf_places_last_error(pl)); return 3; }
    lf_motion_config mc;
    lf_motion_default_config(&mc);
    lf_motion_result res;
    const int32_t kf[2] = { 0, n_frames - 1 };
    rc = lf_places_motion(pl, NULL, &s, n, n_frames, kf, 1, NULL, &mc, 0, &res);
    if (rc) { fprintf(stderr, "lf_places_motion: %d (%s)\n", rc, lf_places_last_error(pl)); return 3; }
    FILE* o = fopen(argv[6], "wb");
    if (!o || fwrite(hits, sizeof(lf_place_hit), nf * (size_t)c.top_k, o) != nf * (size_t)c.top_k || fwrite(scores, sizeof(int32_t), nf * nk, o) != nf * nk ||
        fwrite(&res, sizeof(res), 1, o) != 1) { perror(argv[6]); return 2; }
    fclose(o);
    /* one query too many for the handle is refused, and nothing moves */
    const size_t hit_bytes = nf * (size_t)c.top_k * sizeof(lf_place_hit);
    lf_place_hit* again = (lf_place_hit*)malloc(hit_bytes);
    memcpy(again, hits, hit_bytes);
    rc = lf_places_query(pl, NULL, &s, n, n_frames, frames, n_frames + 1, NULL, &c, 0, again, NULL);
    printf("%d\n%s\n%d\n", rc, lf_places_last_error(pl), memcmp(hits, again, hit_bytes) == 0);
    if (lf_places_clear(pl) != LF_OK || lf_places_count(pl, &count, NULL) != LF_OK || count != 0 || lf_places_synchronize(pl) != LF_OK) return 3;
    lf_places_destroy(pl);
    free(hits); free(again); free(scores); free(frames); free(ground); free(raw);
    return 0;
}
