/* A plain-C client of the front end with the LineDetectorHSV detector (include/lanefront.h, LF_DETECTOR_HOUGH): selects
 * it with the hough_* values of the reference's default.yaml, runs one batch with host outputs and writes the lines.
 *
 *   hough_client <config.bin> <frames.bin> <n_frames> <out.bin>      out.bin: total, frame_offset[n + 1], lines[total][4]
 *
 * Compiled by gcc (C11), no HIP headers: only the C ABI.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lanefront.h"

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
    if (argc != 5) { fprintf(stderr, "usage: hough_client <config.bin> <frames.bin> <n_frames> <out.bin>\n"); return 2; }
    lf_config* cfg = (lf_config*)xread(argv[1], sizeof(lf_config));
    const int n = atoi(argv[3]);
    if (n < 1) { fprintf(stderr, "n_frames must be >= 1\n"); return 2; }
    const size_t frame_bytes = (size_t)cfg->in_rows * cfg->in_cols * 3;
    uint8_t* frames = (uint8_t*)xread(argv[2], frame_bytes * n);
    const int cap_lines = 1024, cap = n * 3 * cap_lines;
    lf_handle* h = NULL;
    int rc = lf_create(cfg, 0, n, cap_lines, &h);
    if (rc) { fprintf(stderr, "lf_create: %d (%s)\n", rc, lf_last_error(NULL)); return 3; }
    lf_hough_params hp;
    lf_hough_default_params(&hp);
    hp.threshold = 2; hp.min_line_length = 3; hp.max_line_gap = 1;
    if ((rc = lf_set_hough_params(h, &hp)) || (rc = lf_set_detector(h, LF_DETECTOR_HOUGH, NULL))) {
        fprintf(stderr, "hough: %d (%s)\n", rc, lf_last_error(h));
        return 4;
    }
    lf_hough_params back;
    if (lf_get_hough_params(h, &back) || back.threshold != 2 || back.min_line_length != 3 || back.max_line_gap != 1) { fprintf(stderr, "lf_get_hough_params\n"); return 5; }
    int32_t* fo = (int32_t*)malloc(sizeof(int32_t) * (n + 1));
    float* lines = (float*)malloc(sizeof(float) * 4 * (size_t)cap);
    lf_segments s;
    memset(&s, 0, sizeof(s));
    s.capacity = cap; s.frame_offset = fo; s.lines = lines;
    int total = 0;
    rc = lf_process_batch(h, frames, n, 0, &s, 0, 0, &total);
    if (rc) { fprintf(stderr, "lf_process_batch: %d (%s)\n", rc, lf_last_error(h)); return 6; }
    FILE* f = fopen(argv[4], "wb");
    if (!f) { perror(argv[4]); return 2; }
    fwrite(&total, sizeof(int32_t), 1, f);
    fwrite(fo, sizeof(int32_t), (size_t)n + 1, f);
    fwrite(lines, sizeof(float) * 4, (size_t)total, f);
    fclose(f);
    lf_destroy(h);
    free(fo); free(lines); free(frames); free(cfg);
    return 0;
}
