/* A plain-C client of include/lanefront.h's loop closures: built with -Werror from the header alone.  Without arguments it prints
 * the sizes of lf_graph_config, lf_graph_result and lf_correct_result as this compiler lays them out and as the library reports
 * them, then the default configuration (lf_map_graph_default_config runs on the host and opens no device).  With the argument
 * "run" it solves a square of four keys with one robust loop edge and prints the solved poses, the chi-squares and the result in
 * hexadecimal floats. */
#include <stdio.h>
#include <string.h>
#include "lanefront.h"

static int run(void)
{
    /* a unit square driven counter-clockwise; the odometry over-turns by 0.05 rad per key, the loop edge says key 3 sees key 0 where it is */
    const double pose[12] = { 0.0, 0.0, 0.0, 1.0, 0.0, 1.62, 1.05, 1.0, 3.24, 0.1, 1.1, 4.86 };
    const int32_t ij[8] = { 0, 1, 1, 2, 2, 3, 3, 0 };
    const double z[12] = { 1.0, 0.0, 1.62, 1.0, 0.0, 1.62, 1.0, 0.0, 1.62, 1.0, 0.0, 1.5707963267948966 };
    const double w[12] = { 100.0, 100.0, 100.0, 100.0, 100.0, 100.0, 100.0, 100.0, 100.0, 400.0, 400.0, 0.0 };
    const uint8_t robust[4] = { 0, 0, 0, 1 };
    double out[12], chi2[4];
    lf_map_config mc;
    lf_map* m = NULL;
    lf_graph_config c;
    lf_graph_result res;
    int k, rc;
    memset(&mc, 0, sizeof(mc));
    mc.capacity = 64; mc.max_distance = 128;
    if ((rc = lf_map_create(0, &mc, &m)) != LF_OK) { fprintf(stderr, "lf_map_create: %s\n", lf_map_last_error(NULL)); return 3; }
    lf_map_graph_default_config(&c);
    c.huber = 0.5;
    rc = lf_map_graph_solve(m, pose, 4, ij, z, w, robust, 4, NULL, &c, out, chi2, &res);
    if (rc != LF_OK) { fprintf(stderr, "lf_map_graph_solve: %s\n", lf_map_last_error(m)); return 4; }
    for (k = 0; k < 4; ++k) printf("%a %a %a %a\n", out[3 * k], out[3 * k + 1], out[3 * k + 2], chi2[k]);
    printf("%a %a %d %d %d %d\n", res.cost0, res.cost, res.status, res.iterations, res.cg_iterations, res.cg_capped);
    lf_map_destroy(m);
    return 0;
}

int main(int argc, char** argv)
{
    lf_graph_config c;
    int (*solve)(lf_map*, const double*, int, const int32_t*, const double*, const double*, const uint8_t*, int, const uint8_t*,
                 const lf_graph_config*, double*, double*, lf_graph_result*) = lf_map_graph_solve;
    int (*correct)(lf_map*, const int32_t*, const double*, const double*, int, lf_correct_result*) = lf_map_correct;
    int (*timing)(lf_map*, double*, int32_t*) = lf_map_graph_timing;
    if (!solve || !correct || !timing) return 2;
    if (argc > 1 && strcmp(argv[1], "run") == 0) return run();
    printf("%d %d %d %d %d\n", (int)sizeof(lf_graph_config), lf_sizeof_graph_config(), (int)sizeof(lf_graph_result), lf_sizeof_graph_result(),
           (int)sizeof(lf_correct_result));
    lf_map_graph_default_config(&c);
    printf("%d %d\n", c.iterations, c.cg_iterations);
    printf("%a %a %f %f %f\n", c.cg_tol, c.damping, c.huber, c.max_shift, c.max_turn);
    return 0;
}
