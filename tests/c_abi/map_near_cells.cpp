// k_map_near.h's host side, built as plain C++: reads lines of "v cell" (hex floats) and prints the cell of v and the cell's size
// for a radius of v, so that tests/test_map_near_cpu.py can hold the kernels' cell function to the Python model of the grid.
#include <stdint.h>
#include <stdio.h>
#include "lanefront.h"
#include "k_map_near.h"

int main()
{
    double v, cell;
    while (scanf("%la %la", &v, &cell) == 2) printf("%d %a\n", (int)lf::nr::cell_of(v, cell), lf::nr::cell_size(v));
    return 0;
}
