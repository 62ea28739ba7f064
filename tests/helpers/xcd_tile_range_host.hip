// Host-side probe of chain_common.h: xcd_tile_range (tests/test_xcd_tile_range.py): reads "nblk ntiles" lines from stdin, prints "t0 tstep tend"
// for every workgroup 0 .. nblk - 1 of each line.  No device code runs.
#include "chain_common.h"
#include <cstdio>
int main() {
    int nblk, ntiles;
    while (scanf("%d %d", &nblk, &ntiles) == 2) {
        for (int bid = 0; bid < nblk; ++bid) {
            int t0, tstep, tend;
            dir::chain::xcd_tile_range(nblk, (unsigned)bid, ntiles, t0, tstep, tend);
            printf("%d %d %d\n", t0, tstep, tend);
        }
    }
    return 0;
}
