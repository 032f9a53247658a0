/* A plain-C client of include/lanefront.h's camera view of the live map: built with -Werror from the header alone.  It prints the
 * size of lf_camera_view as this compiler lays it out and as the library reports it, then the default view of a homography given
 * on the command line as nine numbers (lf_map_camera_view runs on the host and opens no device). */
#include <stdio.h>
#include <stdlib.h>
#include "lanefront.h"

int main(int argc, char** argv)
{
    double H[9];
    lf_camera_view v;
    int (*render)(lf_map*, const lf_camera_view*, const double*, int, const uint8_t*, uint8_t*, int, int32_t*) = lf_map_render_camera;
    int (*timing)(lf_map*, double*, int) = lf_map_render_camera_timing;
    int k, rc;
    if (argc != 10 || !render || !timing) return 2;
    for (k = 0; k < 9; ++k) H[k] = strtod(argv[1 + k], NULL);
    printf("%d %d\n", (int)sizeof(lf_camera_view), lf_sizeof_camera_view());
    rc = lf_map_camera_view(H, 640, 480, 120, 160, 40, &v);
    printf("%d %d %d %d %d %d %d %d %d\n", rc, v.rows, v.cols, v.top_cutoff, v.cam_w, v.cam_h, v.thickness, v.palette_size, (int)v.palette[1][1]);
    for (k = 0; k < 9; ++k) printf("%a\n", v.hinv[k]);
    printf("%a\n", v.w_near);
    return 0;
}
