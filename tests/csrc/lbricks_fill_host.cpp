// lbricks_fill_host.cpp -- stand-alone program around soc_amd/csrc/soc_lbricks.h and the lt_* entry points of tests/ltree_host.cpp
// (TEST CODE, tests/test_lbricks_fill.py): builds the bricks of a hierarchy with either partition, checks them, follows rays
// through them and writes what it found to a file.  A program with its own main, so that -fsanitize=address,undefined needs
// nothing from the process that starts it.
//
//   lbricks_fill_host IN OUT
// IN : int32 NX, NY, NZ, LEVELS, cap, partition, nrays, maxsteps, boxes_only, cells; int32 LCELLS[LEVELS], OFF[LEVELS];
//      float DENS[cells]; float pos[nrays][3], dir[nrays][3]
// OUT: int32 ok, bricks, max_slots, check, slabs, n_tiles, n_slabs, 0; int64 slots; double area_tiles, area_slabs;
//      int32 box[bricks][7] (x0, y0, z0, bx, by, bz, cells); unless boxes_only: int32 rbrick[NX*NY*NZ] and per ray
//      int32 n, status; float end[3]; int32 level[n], cell[n]; float ds[n]
#include <cstdio>
#include <cstdlib>

#include "../ltree_host.cpp"

template <typename T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <typename T> static bool wr(FILE *f, const T *p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]);  return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]);  return 2; }
    int h[10];
    if (!rd(in, h, 10)) return 2;
    const int NX = h[0], NY = h[1], NZ = h[2], LEVELS = h[3], cap = h[4], partition = h[5], nrays = h[6], maxsteps = h[7], boxes_only = h[8], cells = h[9];
    if (NX < 1 || NY < 1 || NZ < 1 || LEVELS < 1 || LEVELS > 16 || cells < 1 || nrays < 0 || maxsteps < 0) return 2;
    std::vector<int> LCELLS(LEVELS), OFF(LEVELS);
    std::vector<float> DENS((size_t)cells), pos((size_t)nrays * 3), dir((size_t)nrays * 3);
    if (!rd(in, LCELLS.data(), LEVELS) || !rd(in, OFF.data(), LEVELS) || !rd(in, DENS.data(), cells) || !rd(in, pos.data(), pos.size()) || !rd(in, dir.data(), dir.size())) return 2;
    fclose(in);
    FILE *out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]);  return 2; }

    Harness *H = new Harness();
    H->NX = NX;  H->NY = NY;  H->NZ = NZ;  H->LEVELS = LEVELS;  H->LCELLS = LCELLS;  H->OFF = OFF;
    soc_lb::Builder::Boxes B;
    bool ok;
    if (boxes_only) {
        soc_lb::Builder bld(NX, NY, NZ, LEVELS, LCELLS.data(), OFF.data(), DENS.data(), cap, H->B);
        ok = bld.boxes(partition, B);
    } else {
        ok = soc_lbricks_build(NX, NY, NZ, LEVELS, LCELLS.data(), OFF.data(), DENS.data(), cap, H->B, partition);
        for (const SocLBrick &K : H->B.bricks) B.push_back(soc_lb::Builder::Box{ K.x0, K.y0, K.z0, K.bx, K.by, K.bz, (uint32_t)K.nslot });
    }
    if (!ok) B.clear();
    const int head[8] = { ok ? 1 : 0, (int)B.size(), H->B.max_slots, (ok && !boxes_only) ? lt_check(H, DENS.data(), cells) : 0,
                          H->B.slabs ? 1 : 0, H->B.n_tiles, H->B.n_slabs, 0 };
    const long long slots = (long long)H->B.btree.size();
    const double areas[2] = { H->B.area_tiles, H->B.area_slabs };
    bool good = wr(out, head, 8) && wr(out, &slots, 1) && wr(out, areas, 2);
    for (const auto &b : B) { const int v[7] = { b.x0, b.y0, b.z0, b.dx, b.dy, b.dz, (int)b.n };  good = good && wr(out, v, 7); }
    if (ok && !boxes_only) {
        good = good && wr(out, H->B.rbrick.data(), H->B.rbrick.size());
        std::vector<int> lev((size_t)maxsteps), cel((size_t)maxsteps);
        std::vector<float> ds((size_t)maxsteps);
        for (int r = 0; r < nrays && good; r++) {
            float end[3];
            int st = 0;
            const int n = lt_trace_move(H, &pos[3 * (size_t)r], &dir[3 * (size_t)r], maxsteps, lev.data(), cel.data(), ds.data(), end, &st);
            const int ns[2] = { n, st };
            good = wr(out, ns, 2) && wr(out, end, 3) && wr(out, lev.data(), n) && wr(out, cel.data(), n) && wr(out, ds.data(), n);
        }
    }
    delete H;
    if (fclose(out) != 0 || !good) { fprintf(stderr, "write failed\n");  return 2; }
    return 0;
}
