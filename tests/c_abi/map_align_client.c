/* A plain-C client of include/lanefront.h's pose alignment against the live map: built with -Werror from the header alone.  It
 * prints the sizes of lf_align_config and lf_align_result as this compiler lays them out and as the library reports them, then
 * the default configuration (lf_map_align_default_config runs on the host and opens no device). */
#include <stdio.h>
#include "lanefront.h"

int main(void)
{
    lf_align_config c;
    int (*align)(lf_map*, lf_handle*, const lf_segments*, int, int, const int32_t*, const float*, const double*, const lf_align_config*, int,
                 lf_align_result*) = lf_map_align;
    int (*step)(lf_map*, lf_handle*, const lf_segments*, int, int, const double*, const lf_align_config*, int, int32_t*, float*,
                lf_align_result*) = lf_map_step_aligned;
    int (*step_host)(lf_map*, const lf_segments*, int, int, const double*, const lf_align_config*, int, int32_t*, float*,
                     lf_align_result*) = lf_map_step_aligned_host;
    int (*timing)(lf_map*, double*, int32_t*) = lf_map_align_timing;
    if (!align || !step || !step_host || !timing) return 2;
    printf("%d %d %d %d\n", (int)sizeof(lf_align_config), lf_sizeof_align_config(), (int)sizeof(lf_align_result), lf_sizeof_align_result());
    lf_map_align_default_config(&c);
    printf("%d %d %d %d\n", c.iterations, c.min_pairs, c.min_hits, c.color_match);
    printf("%a %f %f %a %a %f %f\n", c.gate, c.huber, c.max_dist, c.prior_xy, c.prior_theta, c.max_shift, c.max_turn);
    printf("%d %d %d %d\n", LF_ALIGN_OK, LF_ALIGN_FEW, LF_ALIGN_DEGENERATE, LF_ALIGN_REJECTED);
    return 0;
}
