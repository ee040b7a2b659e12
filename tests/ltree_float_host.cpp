// ltree_float_host.cpp -- host harness for the FLOAT form of soc_amd/csrc/soc_ltree.h (TEST CODE): follows rays through the
// brick-local hierarchies as the device walk does on grids whose Index() the reference evaluates with float3 POS (GetStep's float
// arithmetic, then soc_lt_aim_flt / soc_lt_land_flt) and reports every step, so that tests/test_ltree_float.py can compare it
// with the oracle's IndexG/GetStep/Index (oracle/soc_oracle.c, float Index) step by step.  Built by the test with g++ as a shared
// library; with -DLTF_MAIN as a stand-alone program (built with sanitizers) that reads a cloud and rays from a file.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../soc_amd/csrc/soc_lbricks.h"

#define PEPS 1.0e-4f

struct Harness {
    int NX, NY, NZ, LEVELS;
    SocLBricksHost B;
};

extern "C" {

void *ltf_build(int NX, int NY, int NZ, int LEVELS, const int *LCELLS, const int *OFF, const float *DENS, int cap)
{
    Harness *H = new Harness();
    H->NX = NX;  H->NY = NY;  H->NZ = NZ;  H->LEVELS = LEVELS;
    if (!soc_lbricks_build(NX, NY, NZ, LEVELS, LCELLS, OFF, DENS, cap, H->B)) { delete H;  return nullptr; }
    return H;
}

void ltf_free(void *h) { delete (Harness *)h; }

int ltf_info(void *h, int *nbricks, int *max_slots, long *nslots)
{
    Harness *H = (Harness *)h;
    *nbricks = (int)H->B.bricks.size();  *max_slots = H->B.max_slots;  *nslots = (long)H->B.btree.size();
    return 0;
}

// the leaf that holds a point of the root grid (IndexG = the arrival of a root-level packet): level, coordinates on that level and
// the local position.  Returns the outcome of the move.
int ltf_locate(void *h, const float *pos, int *level, int *c, float *local)
{
    Harness *H = (Harness *)h;
    const int NX = H->NX, NY = H->NY, NZ = H->NZ, Lmax = H->LEVELS - 1;
    float px = pos[0], py = pos[1], pz = pos[2], dens = 0.0f;
    if ((px <= 0.0f) || (py <= 0.0f) || (pz <= 0.0f) || (px >= NX) || (py >= NY) || (pz >= NZ)) return SOC_LT_EXIT;
    const SocLBrick &K = H->B.bricks[H->B.rbrick[((int)floorf(pz) * NY + (int)floorf(py)) * NX + (int)floorf(px)]];
    int lv = 0, cx = 0, cy = 0, cz = 0, slot = -1, obase = -1, Rx, Ry, Rz;
    const int r = soc_lt_move<true>(H->B.btree.data() + K.base, K, NX, NY, NZ, Lmax, 0, SOC_LTM_ARRIVE, px, py, pz, lv, cx, cy, cz, slot, obase, dens, Rx, Ry, Rz);
    *level = lv;  c[0] = cx;  c[1] = cy;  c[2] = cz;  local[0] = px;  local[1] = py;  local[2] = pz;
    return r;
}

// One Index() of the float form for a packet in cell (level, c) whose position after GetStep is `pos` (local to the cell's octet):
// the cell is placed in its brick, then the step is made.  Returns the outcome; level, c and pos are the new place when it is INSIDE.
int ltf_step(void *h, int *level, int *c, float *pos)
{
    Harness *H = (Harness *)h;
    const int NX = H->NX, NY = H->NY, NZ = H->NZ, Lmax = H->LEVELS - 1;
    const int rx = c[0] >> *level, ry = c[1] >> *level, rz = c[2] >> *level;
    if (rx < 0 || ry < 0 || rz < 0 || rx >= NX || ry >= NY || rz >= NZ) return -1;
    const SocLBrick &K = H->B.bricks[H->B.rbrick[(rz * NY + ry) * NX + rx]];
    const float *tree = H->B.btree.data() + K.base;
    int lv = *level, cx = c[0], cy = c[1], cz = c[2], slot = -1, obase = -1, Rx, Ry, Rz;
    float px = pos[0], py = pos[1], pz = pos[2], dens = 0.0f;
    int r = soc_lt_move<true>(tree, K, NX, NY, NZ, Lmax, 0, SOC_LTM_PLACE, px, py, pz, lv, cx, cy, cz, slot, obase, dens, Rx, Ry, Rz);
    if (r != SOC_LT_INSIDE) return -2;
    r = soc_lt_move<true>(tree, K, NX, NY, NZ, Lmax, 0, SOC_LTM_STEP, px, py, pz, lv, cx, cy, cz, slot, obase, dens, Rx, Ry, Rz);
    *level = lv;  c[0] = cx;  c[1] = cy;  c[2] = cz;  pos[0] = px;  pos[1] = py;  pos[2] = pz;
    return r;
}

// Follow one ray through soc_lt_move<true>(), the single-path form the device walk uses: steps, arrivals in the next brick and --
// after every move -- a placement of the packet's own cell, which must find the slot and the density the move reported.
// Per step: level, global cell index, step length (root units), as orc_trace reports them.  Returns the number of steps;
// *status: 0 left the model, 1 maxsteps, 2 stopped at a step that needs the generic Index, -1 lost, -3 a placement disagreed.
int ltf_trace_move(void *h, const float *pos, const float *dir, int maxsteps, int *levels, int *cells, float *dss, float *endpos, int *status)
{
    Harness *H = (Harness *)h;
    const int NX = H->NX, NY = H->NY, NZ = H->NZ, Lmax = H->LEVELS - 1;
    const int kexp = 0;                                     // (the float form has no use for it)
    float px = pos[0], py = pos[1], pz = pos[2];
    const float ux = dir[0], uy = dir[1], uz = dir[2];
    int level = 0, cx = 0, cy = 0, cz = 0, slot = -1, obase = -1, n = 0, Rx, Ry, Rz;
    float dens = 0.0f;
    *status = 0;
    endpos[0] = px;  endpos[1] = py;  endpos[2] = pz;
    if ((px <= 0.0f) || (py <= 0.0f) || (pz <= 0.0f) || (px >= NX) || (py >= NY) || (pz >= NZ)) return 0;      // IndexG
    int brick = H->B.rbrick[((int)floorf(pz) * NY + (int)floorf(py)) * NX + (int)floorf(px)];
    int what = SOC_LTM_ARRIVE;                              // IndexG = an arrival of a root-level packet
    while (true) {
        const SocLBrick &K = H->B.bricks[brick];
        const float *tree = H->B.btree.data() + K.base;
        if (what == SOC_LTM_STEP) {
            if (n >= maxsteps) { *status = 1;  break; }
            levels[n] = level;
            cells[n]  = H->B.bcell[K.base + slot];
            const float ax = (ux > 0.0f) ? (((1.0f + PEPS) - soc_fmod1f(px)) / ux) : ((-PEPS - soc_fmod1f(px)) / ux);
            const float ay = (uy > 0.0f) ? (((1.0f + PEPS) - soc_fmod1f(py)) / uy) : ((-PEPS - soc_fmod1f(py)) / uy);
            const float az = (uz > 0.0f) ? (((1.0f + PEPS) - soc_fmod1f(pz)) / uz) : ((-PEPS - soc_fmod1f(pz)) / uz);
            const float s = soc_fminf(ax, soc_fminf(ay, az));
            px += s * ux;  py += s * uy;  pz += s * uz;
            dss[n] = soc_scale_down(s, level);
            n++;
        }
        const int L0 = level, c0x = cx, c0y = cy, c0z = cz;
        const int r = soc_lt_move<true>(tree, K, NX, NY, NZ, Lmax, kexp, what, px, py, pz, level, cx, cy, cz, slot, obase, dens, Rx, Ry, Rz);
        if (r == SOC_LT_EXIT) {
            soc_lt_rootpos_f(px, py, pz, L0, c0x, c0y, c0z);      // Index() leaves the root-grid position behind (kernel_ASOC_aux.c:230-233)
            break;
        }
        if (r == SOC_LT_SLOW) { *status = 2;  break; }
        if (r == SOC_LT_LOST) { *status = -1;  break; }
        if (r == SOC_LT_LEAVE) {
            brick = H->B.rbrick[(Rz * NY + Ry) * NX + Rx];
            what = SOC_LTM_ARRIVE;
            slot = obase = -1;                                 // (they mean nothing in the next brick)
            continue;
        }
        {   // placement of the cell just found
            int s2 = -1, b2 = -1, l2 = level, ax2 = cx, ay2 = cy, az2 = cz, qx, qy, qz;
            float d2 = 0.0f, p2x = px, p2y = py, p2z = pz;
            const int r2 = soc_lt_move<true>(tree, K, NX, NY, NZ, Lmax, kexp, SOC_LTM_PLACE, p2x, p2y, p2z, l2, ax2, ay2, az2, s2, b2, d2, qx, qy, qz);
            if (r2 != SOC_LT_INSIDE || s2 != slot || d2 != dens || l2 != level || p2x != px || (level > 0 && b2 != obase)) { *status = -3;  break; }
        }
        what = SOC_LTM_STEP;
    }
    endpos[0] = px;  endpos[1] = py;  endpos[2] = pz;
    return n;
}

}  // extern "C"

#if defined(LTF_MAIN)
// Stand-alone run (sanitizer build): the file holds, as 32-bit words, NX NY NZ LEVELS cap nrays | LCELLS[LEVELS] | OFF[LEVELS] |
// DENS[cells] (float) | nrays x (pos[3], dir[3]) (float).  Builds the bricks, follows every ray, prints totals.
template <typename T> static bool rd(FILE *f, std::vector<T> &v, size_t n) { v.resize(n);  return fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s file\n", argv[0]);  return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]);  return 2; }
    std::vector<int> hd, lc, off;
    std::vector<float> dens, rays;
    bool ok = rd(f, hd, 6);
    if (ok && (hd[3] < 1 || hd[3] > 8 || hd[5] < 0)) ok = false;
    ok = ok && rd(f, lc, hd[3]) && rd(f, off, hd[3]);
    long cells = 0;
    for (int l = 0; ok && l < hd[3]; l++) cells += lc[l];
    ok = ok && rd(f, dens, (size_t)cells) && rd(f, rays, (size_t)hd[5] * 6);
    fclose(f);
    if (!ok) { fprintf(stderr, "short or malformed file\n");  return 2; }
    void *h = ltf_build(hd[0], hd[1], hd[2], hd[3], lc.data(), off.data(), dens.data(), hd[4]);
    if (!h) { printf("bricks refused\n");  return 0; }
    const int maxsteps = 20000;
    std::vector<int> lev(maxsteps), cel(maxsteps);
    std::vector<float> ds(maxsteps);
    long steps = 0;
    int slow = 0, bad = 0;
    for (int i = 0; i < hd[5]; i++) {
        float end[3];
        int st = 0;
        steps += ltf_trace_move(h, &rays[6 * (size_t)i], &rays[6 * (size_t)i + 3], maxsteps, lev.data(), cel.data(), ds.data(), end, &st);
        slow += (st == 2);  bad += (st != 0 && st != 2);
        int l2, c2[3];
        float loc[3];
        ltf_locate(h, &rays[6 * (size_t)i], &l2, c2, loc);
    }
    int nb, ms;
    long ns;
    ltf_info(h, &nb, &ms, &ns);
    ltf_free(h);
    printf("rays %d steps %ld slow %d bad %d bricks %d slots %ld\n", hd[5], steps, slow, bad, nb, ns);
    return bad ? 1 : 0;
}
#endif
