/* A plain-C client of the histogram lane filter (include/lanefront.h "Histogram lane filter"): what the lane_filter
 * node's integrator links against.  Reads raw frames and per-frame (dt, v, w) written by tests/test_lane_filter_cpu.py /
 * tests/test_gpu_lane_filter.py, runs the front end with host outputs, then one filter stream over the frames, and writes
 * the poses (lf_lane_pose per frame) back.
 *
 *   lane_filter_client <config.bin> <frames.bin> <n_frames> <dtvw.bin> <poses.bin>
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
    if (argc != 6) { fprintf(stderr, "usage: lane_filter_client <config.bin> <frames.bin> <n_frames> <dtvw.bin> <poses.bin>\n"); return 2; }
    lf_config* cfg = (lf_config*)xread(argv[1], sizeof(lf_config));
    const int n = atoi(argv[3]);
    if (n < 1) { fprintf(stderr, "n_frames must be >= 1\n"); return 2; }
    const size_t frame_bytes = (size_t)cfg->in_rows * cfg->in_cols * 3;
    uint8_t* frames = (uint8_t*)xread(argv[2], frame_bytes * n);
    double* dtvw = (double*)xread(argv[4], sizeof(double) * 3 * n);
    const int cap_lines = 1024, cap = n * 3 * cap_lines;
    lf_handle* h = NULL;
    int rc = lf_create(cfg, 0, n, cap_lines, &h);
    if (rc) { fprintf(stderr, "lf_create: %d (%s)\n", rc, lf_last_error(NULL)); return 3; }
    lf_segments s;
    memset(&s, 0, sizeof(s));
    s.capacity = cap;
    s.frame_offset = (int32_t*)calloc(n + 1, sizeof(int32_t));
    s.color = (uint8_t*)calloc(cap, 1);
    s.ground = (double*)calloc((size_t)cap * 4, sizeof(double));
    int total = 0;
    rc = lf_process_batch(h, frames, n, 0, &s, 0, 0, &total);
    if (rc) { fprintf(stderr, "lf_process_batch: %d (%s)\n", rc, lf_last_error(h)); return 3; }
    lf_lane_filter_config lc;
    lf_lane_filter_default_config(&lc);
    lf_lane_filter* lf = NULL;
    rc = lf_lane_filter_create(0, &lc, 1, n, &lf);
    if (rc) { fprintf(stderr, "lf_lane_filter_create: %d (%s)\n", rc, lf_lane_filter_last_error(NULL)); return 3; }
    lf_lane_pose* poses = (lf_lane_pose*)calloc(n, sizeof(lf_lane_pose));
    rc = lf_lane_filter_step(lf, NULL, &s, 0, n, NULL, dtvw, LF_LANE_FILTER_PREDICT | LF_LANE_FILTER_UPDATE, poses, NULL, NULL);
    if (rc) { fprintf(stderr, "lf_lane_filter_step: %d (%s)\n", rc, lf_lane_filter_last_error(lf)); return 3; }
    FILE* o = fopen(argv[5], "wb");
    if (!o || fwrite(poses, sizeof(lf_lane_pose), n, o) != (size_t)n) { perror(argv[5]); return 2; }
    fclose(o);
    printf("%d frames, %d segments\n", n, total);
    lf_lane_filter_destroy(lf);
    lf_destroy(h);
    free(poses); free(s.frame_offset); free(s.color); free(s.ground); free(frames); free(dtvw); free(cfg);
    return 0;
}
