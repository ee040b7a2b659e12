// ltree_diet_host.cpp -- stand-alone host check of the integer forms of soc_ltree.h that replaced longer expressions: the new form against the
// old expression (kept here, not in the product), equality of every result, no tolerance.  Built with -fsanitize=address,undefined and run as a
// program (tests/test_ltree_diet.py).
//
//   soc_lt_octant / the sibling slot of soc_lt_aim: for a sibling move J = floor(pos * 2^D) lies below 2^(D+1) on every axis, so J >> D is the
//   octant bit and needs no mask.  soc_lt_octant: every J triple of a sibling for every D <= 7 (exhaustive).  Through soc_lt_aim itself:
//   every (Lmax, level) with Lmax <= 7, A.s of a sibling move equals obase + the old expression, on every J triple where 2^(D+1) <= 32 and
//   on a lattice of 32 values per axis above that (all octants, J >> D and the bits below D varying).
#include <cstdio>
#include <cstdlib>
#include "soc_ltree.h"

static int old_octant(int Jx, int Jy, int Jz, int D) { return ((Jx >> D) & 1) | (((Jy >> D) & 1) << 1) | (((Jz >> D) & 1) << 2); }

int main()
{
    long checked = 0, aimed = 0;
    // every octant-bit triple, and every sibling J of every D
    for (int D = 0; D <= 7; D++) {
        const int n = 1 << (D + 1);
        for (int Jz = 0; Jz < n; Jz++)
            for (int Jy = 0; Jy < n; Jy++)
                for (int Jx = 0; Jx < n; Jx++) {
                    const int want = old_octant(Jx, Jy, Jz, D);
                    const int got = (int)soc_lt_octant((unsigned)Jx >> D, (unsigned)Jy >> D, (unsigned)Jz >> D);
                    if (got != want) { std::printf("octant: D %d J %d %d %d: %d, expected %d\n", D, Jx, Jy, Jz, got, want);  return 1; }
                    checked++;
                }
    }
    // through soc_lt_aim: every (Lmax, level) with Lmax <= 7, positions on a lattice of the octet [0,2)^3 (never on a face, never tiny)
    SocLBrick K;  K.x0 = 2;  K.y0 = 3;  K.z0 = 1;  K.bx = 4;  K.by = 3;  K.bz = 5;  K.base = 0;  K.nslot = 1 << 20;
    for (int Lmax = 1; Lmax <= 7; Lmax++)
        for (int level = 1; level <= Lmax; level++) {
            const int D = Lmax - level, m = 1 << (D + 1);
            const int step = (m > 32) ? (m / 32) : 1;
            for (int iz = 0; iz < m; iz += step)
                for (int iy = 0; iy < m; iy += step)
                    for (int ix = 0; ix < m; ix += step) {
                        // pos = (i + 0.37) / 2^D: floor(pos * 2^D) = i exactly (the scaling is by a power of two)
                        const float sc = soc_lt_pow2(-D);
                        const float px = ((float)ix + 0.37f) * sc, py = ((float)iy + 0.37f) * sc, pz = ((float)iz + 0.37f) * sc;
                        const int cx = (3 << level) | 5, cy = (4 << level) | 2, cz = (2 << level) | 7, obase = 4096 + 8 * level;
                        SocLtAim A;
                        soc_lt_aim(K, 16, 16, 16, Lmax, 4 - 30, SOC_LTM_STEP, px, py, pz, level, cx, cy, cz, obase, A);
                        if (A.r != SOC_LT_INSIDE || A.l != level || A.s != obase + old_octant(ix, iy, iz, D)) {
                            std::printf("aim: Lmax %d level %d i %d %d %d: r %d l %d s %d, expected s %d\n", Lmax, level, ix, iy, iz, A.r, A.l, A.s,
                                        obase + old_octant(ix, iy, iz, D));
                            return 1;
                        }
                        aimed++;
                    }
        }
    std::printf("ltree diet ok: %ld octants, %ld sibling moves\n", checked, aimed);
    return 0;
}
