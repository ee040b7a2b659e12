// Host harness of tests/test_cbricks.py: the brick cutter of single-level grids (soc_amd/csrc/soc_lbricks.h: soc_cbricks_build)
// behind a C interface.  Compiled by the test with g++.
#include "../soc_amd/csrc/soc_lbricks.h"

extern "C" {

void *cb_build(int NX, int NY, int NZ, const float *DENS, int edge)
{
    SocLBricksHost *H = new SocLBricksHost();
    soc_cbricks_build(NX, NY, NZ, DENS, edge, *H);
    return H;
}
void cb_free(void *h) { delete (SocLBricksHost *)h; }
int cb_ok(const void *h) { return ((const SocLBricksHost *)h)->ok ? 1 : 0; }
int cb_nbricks(const void *h) { return (int)((const SocLBricksHost *)h)->bricks.size(); }
int cb_max_slots(const void *h) { return ((const SocLBricksHost *)h)->max_slots; }
long cb_nslots(const void *h) { return (long)((const SocLBricksHost *)h)->btree.size(); }
// boxes: 8 ints per brick (x0, y0, z0, bx, by, bz, base, nslot); rbrick: one int per root cell; bcell, btree: one entry per slot
void cb_read(const void *h, int *boxes, int *rbrick, int *bcell, float *btree)
{
    const SocLBricksHost &H = *(const SocLBricksHost *)h;
    for (size_t b = 0; b < H.bricks.size(); b++) {
        const SocLBrick &K = H.bricks[b];
        const int v[8] = { K.x0, K.y0, K.z0, K.bx, K.by, K.bz, K.base, K.nslot };
        for (int i = 0; i < 8; i++) boxes[8 * b + i] = v[i];
    }
    for (size_t i = 0; i < H.rbrick.size(); i++) rbrick[i] = H.rbrick[i];
    for (size_t i = 0; i < H.bcell.size(); i++) { bcell[i] = H.bcell[i];  btree[i] = H.btree[i]; }
}

}
