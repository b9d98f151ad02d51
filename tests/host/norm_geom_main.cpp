// The geometry of the row-mapped normalisation kernels (norm_common.h: norm_geom, norm_apply_chunk) over a sweep of
// channel counts, batch sizes and voxel counts.  One line per (C, N, V):
//   C N V vec CG R threads nblk chunk achunk(cap 8192 / N) achunk(cap 65535)
// tests/test_norm_geom_host.py runs it and compares with the Python restatement.
#include "norm_common.h"

#include <stdio.h>

using namespace mvd;

int main() {
    const int CS[] = {1, 3, 4, 5, 32, 255, 256, 320, 1023, 1024}, NS[] = {1, 2, 3, 2048, 4096};
    const long VS[] = {1, 7, 511, 512, 4096, 8448, 2097152};
    for (int C : CS)
        for (int N : NS)
            for (long V : VS) {
                const NormGeom g = norm_geom(N, V, C);
                if (g.C != C || g.V != V) return 1;
                printf("%d %d %ld %d %d %d %d %d %ld %ld %ld\n", C, N, V, g.vec, g.CG, g.R, g.threads, g.nblk, g.chunk,
                       norm_apply_chunk(g, 8192 / N), norm_apply_chunk(g, 65535));
            }
    return 0;
}
