// soc_lbricks.h -- host-side construction of the brick-local hierarchies of soc_ltree.h, and of the bricks of root cells of
// single-level grids (soc_cbricks_build, at the end).  Plain C++ (no HIP), so the
// same code is compiled into libsoc_hip.so and -- with -fsanitize=address,undefined -- into the CPU tests.
//
// A brick is a box of root cells together with everything below them, at most `cap` cells (leaves and refined
// cells).  A packet pays for every brick it enters, and for straight paths the number of visits goes with the total
// face area of the boxes, so the boxes are chosen for the smallest total area.  Two partitions of the root grid are
// computed, as lists of boxes only, and the one with the smaller total face area is built (a tie: the first):
//   * tiles: the root grid is cut into tiles of 16^3 cells; a tile that holds more than `cap` cells is halved along
//     its longest edge until every part fits (SOC_LB_TILES builds this one alone);
//   * slabs: a node -- at first the whole grid -- that holds more than SOC_LB_NODE x cap cells is cut in two along its
//     longest edge where half of its cells lie on either side; a smaller node with a clump in it (the cells per root
//     cell of its octants differ by more than SOC_LB_SKEW) is halved along its longest edge.  What is left is a node
//     of about one density, its own, and is cut into slabs along z, each slab into columns along y and each column
//     into boxes along x.  The slabs hold equal numbers of cells and would be e = cbrt(cap / rho) thick if every box
//     were a cube filled to `cap`, rho the cells per root cell of THIS node; the columns of a slab hold equal numbers
//     and would be sqrt(cap A / n) wide, A the slab's face and n its cells (a square column filled to `cap`); a column is cut into the fewest boxes
//     of <= cap cells, as even as its planes allow.  Planes are whole root cells and the cells are not spread evenly,
//     so the numbers of slabs and of columns are tried from that ideal up to boxes filled to 3/4, every slab choosing
//     for itself, and the smallest area is kept; a node thinner than three such boxes is tried with the axes in all
//     six orders.  A piece that still holds more than cap cells (one plane of a column) is a node again; a node
//     that cannot be cut this way (one plane thick on the last axis) is halved.
//   Every profile along an axis is one pass over the node's root cells: no table of the whole grid.
// Within a brick the cells get slots: the root cells of the box first
// (x fastest), then the octets of refined cells in breadth-first order, eight consecutive slots per octet; the
// entry of a refined cell is the link to the first slot of its octet in the cloud file's encoding
// (-(float with the bits of the index)), the entry of a leaf is its density.
#ifndef SOC_LBRICKS_H
#define SOC_LBRICKS_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "soc_ltree.h"

struct SocLBricksHost {
    std::vector<SocLBrick> bricks;
    std::vector<float>     btree;      // [cells with a slot] density or local link
    std::vector<int>       bcell;      // [cells with a slot] global cell index
    std::vector<int>       rbrick;     // [NX*NY*NZ] brick of every root cell
    int  max_slots = 0;
    bool ok = false;                   // false: some root cell holds more than cap cells (or a link is broken)
    // the two partitions (soc_lb::Builder::build): total face area of the boxes, in faces of root cells, and their number;
    // of the one that was not computed (SOC_LB_TILES) 0
    double area_tiles = 0.0, area_slabs = 0.0;
    int    n_tiles = 0, n_slabs = 0;
    bool   slabs = false;              // the bricks are the slab partition's
};

// which partition soc_lbricks_build makes: the one of the two with the smaller face area, or the tiles alone
enum { SOC_LB_BEST = 0, SOC_LB_TILES = 1 };
#ifndef SOC_LB_SKEW
#define SOC_LB_SKEW 2.0                // slabs: a node whose octants differ in cells per root cell by more than this factor is halved
#endif
#ifndef SOC_LB_NODE
#define SOC_LB_NODE 4096               // slabs: a node with more than this many times `cap` cells is cut in two first
#endif

namespace soc_lb {

inline int link_of(float d) { float m = -d;  int i;  memcpy(&i, &m, 4);  return i; }
inline float link_to(int i) { float m;  memcpy(&m, &i, 4);  return -m; }

struct Builder {
    int NX, NY, NZ, LEVELS, cap;
    const int *LCELLS, *OFF;
    const float *D;
    std::vector<uint32_t> sub;         // cells in the subtree of every root cell (saturating)
    SocLBricksHost &out;

    Builder(int nx, int ny, int nz, int levels, const int *lcells, const int *off, const float *dens, int cap_, SocLBricksHost &o)
        : NX(nx), NY(ny), NZ(nz), LEVELS(levels), cap(cap_), LCELLS(lcells), OFF(off), D(dens), out(o) {}

    bool count()
    {
        // cells per subtree, bottom-up over the levels; only the root level is kept
        std::vector<uint32_t> below, cur;
        for (int l = LEVELS - 1; l >= 0; l--) {
            cur.assign((size_t)LCELLS[l], 1u);
            const float *d = D + OFF[l];
            for (int i = 0; i < LCELLS[l]; i++) {
                if (d[i] > 0.0f) continue;
                if (l + 1 >= LEVELS) return false;                   // a link on the last level
                const int c = link_of(d[i]);
                if (c < 0 || c + 8 > LCELLS[l + 1]) return false;
                uint64_t n = 1;
                for (int k = 0; k < 8; k++) n += below[(size_t)c + k];
                cur[i] = (uint32_t)(n > 0x7fffffffu ? 0x7fffffffu : n);
            }
            below.swap(cur);
        }
        sub.swap(below);
        return true;
    }
    uint64_t cells_in(int x0, int y0, int z0, int dx, int dy, int dz) const
    {
        uint64_t n = 0;
        for (int z = z0; z < z0 + dz; z++)
            for (int y = y0; y < y0 + dy; y++) {
                const uint32_t *row = sub.data() + ((size_t)z * NY + y) * NX;
                for (int x = x0; x < x0 + dx; x++) n += row[x];
            }
        return n;
    }
    bool emit(int x0, int y0, int z0, int dx, int dy, int dz, int n)
    {
        SocLBrick K;
        K.x0 = x0;  K.y0 = y0;  K.z0 = z0;  K.bx = dx;  K.by = dy;  K.bz = dz;
        K.base = (int)out.btree.size();
        K.nslot = n;
        const int id = (int)out.bricks.size();
        const size_t base = out.btree.size();
        out.btree.resize(base + n);
        out.bcell.resize(base + n);
        // (global cell, level) of every slot; refined cells are expanded in slot order: breadth first
        std::vector<int> lev((size_t)n);
        int fill = 0;
        for (int z = z0; z < z0 + dz; z++)
            for (int y = y0; y < y0 + dy; y++)
                for (int x = x0; x < x0 + dx; x++) {
                    const int r = (z * NY + y) * NX + x;
                    out.rbrick[r] = id;
                    out.bcell[base + fill] = r;
                    lev[fill] = 0;
                    fill++;
                }
        for (int s = 0; s < fill; s++) {
            const int g = out.bcell[base + s];
            const float d = D[g];
            if (d > 0.0f) { out.btree[base + s] = d;  continue; }
            if (fill + 8 > n) return false;
            const int l = lev[s], c = OFF[l + 1] + link_of(d);
            out.btree[base + s] = link_to(fill);
            for (int k = 0; k < 8; k++) { out.bcell[base + fill] = c + k;  lev[fill] = l + 1;  fill++; }
        }
        if (fill != n) return false;
        out.bricks.push_back(K);
        if (n > out.max_slots) out.max_slots = n;
        return true;
    }
    struct Box { int x0, y0, z0, dx, dy, dz;  uint32_t n; };
    typedef std::vector<Box> Boxes;

    static double area(const Boxes &B)
    {
        double a = 0.0;
        for (const Box &b : B) a += 2.0 * ((double)b.dx * b.dy + (double)b.dy * b.dz + (double)b.dz * b.dx);
        return a;
    }
    static Box sub_box(const Box &b, int axis, int a0, int a1, uint64_t n)
    {
        Box c = b;
        if (axis == 0) { c.x0 = b.x0 + a0;  c.dx = a1 - a0; } else if (axis == 1) { c.y0 = b.y0 + a0;  c.dy = a1 - a0; } else { c.z0 = b.z0 + a0;  c.dz = a1 - a0; }
        c.n = (uint32_t)(n > 0xffffffffu ? 0xffffffffu : n);
        return c;
    }

    // ---- tiles, halved ----
    bool split(int x0, int y0, int z0, int dx, int dy, int dz, Boxes &B) const
    {
        const uint64_t n = cells_in(x0, y0, z0, dx, dy, dz);
        if (n <= (uint64_t)cap) { B.push_back(Box{ x0, y0, z0, dx, dy, dz, (uint32_t)n });  return true; }
        if (dx == 1 && dy == 1 && dz == 1) return false;             // one root cell with more than cap cells below it
        if (dz >= dy && dz >= dx) { const int h = (dz + 1) / 2;  return split(x0, y0, z0, dx, dy, h, B) && split(x0, y0, z0 + h, dx, dy, dz - h, B); }
        if (dy >= dx)             { const int h = (dy + 1) / 2;  return split(x0, y0, z0, dx, h, dz, B) && split(x0, y0 + h, z0, dx, dy - h, dz, B); }
        const int h = (dx + 1) / 2;
        return split(x0, y0, z0, h, dy, dz, B) && split(x0 + h, y0, z0, dx - h, dy, dz, B);
    }
    bool tiles(Boxes &B) const
    {
        const int T = 16;
        for (int z = 0; z < NZ; z += T)
            for (int y = 0; y < NY; y += T)
                for (int x = 0; x < NX; x += T) {
                    const int dx = (x + T <= NX) ? T : NX - x, dy = (y + T <= NY) ? T : NY - y, dz = (z + T <= NZ) ? T : NZ - z;
                    if (!split(x, y, z, dx, dy, dz, B)) return false;
                }
        return true;
    }

    // ---- slabs, columns, boxes ----
    // P[i] = cells of the box in its planes 0 .. i-1 along `axis` (P[0] = 0, P[len] = all): one pass over its root cells
    void profile(const Box &b, int axis, std::vector<uint64_t> &P) const
    {
        const int len = (axis == 0) ? b.dx : (axis == 1) ? b.dy : b.dz;
        P.assign((size_t)len + 1, 0);
        for (int z = 0; z < b.dz; z++)
            for (int y = 0; y < b.dy; y++) {
                const uint32_t *row = sub.data() + ((size_t)(b.z0 + z) * NY + (b.y0 + y)) * NX + b.x0;
                if (axis == 0) for (int x = 0; x < b.dx; x++) P[x + 1] += row[x];
                else { uint64_t n = 0;  for (int x = 0; x < b.dx; x++) n += row[x];  P[(axis == 1 ? y : z) + 1] += n; }
            }
        for (int i = 0; i < len; i++) P[i + 1] += P[i];
    }
    // the plane in [lo, hi] whose running count is nearest to `want` (the lower one of two equally near)
    static int nearest(const std::vector<uint64_t> &P, int lo, int hi, double want)
    {
        int a = lo, b = hi;
        while (a < b) { const int m = (a + b) / 2;  if ((double)P[m] < want) a = m + 1; else b = m; }
        if (a > lo && want - (double)P[a - 1] <= (double)P[a] - want) a--;
        return a;
    }
    // k pieces of about equal count, each at least one plane thick: C = 0, ..., len
    static void even_cuts(const std::vector<uint64_t> &P, int k, std::vector<int> &C)
    {
        const int len = (int)P.size() - 1;
        C.assign(1, 0);
        for (int i = 1; i < k; i++) C.push_back(nearest(P, C.back() + 1, len - (k - i), (double)P[len] * i / k));
        C.push_back(len);
    }
    // the fewest pieces of <= cap cells, as even as the planes allow.  A plane that holds more than cap cells by itself is a piece.
    void capped_cuts(const std::vector<uint64_t> &P, std::vector<int> &C) const
    {
        const int len = (int)P.size() - 1;
        std::vector<int> G(1, 0);                                     // greedy: every piece as long as cap lets it be
        while (G.back() < len) {
            int c = G.back() + 1;
            while (c < len && P[c + 1] - P[G.back()] <= (uint64_t)cap) c++;
            G.push_back(c);
        }
        const int k = (int)G.size() - 1;
        C.assign(1, 0);
        bool fits = true;
        for (int i = 1; i < k && fits; i++) {
            const int lo = C.back() + 1, hi = len - (k - i);
            if (lo > hi) { fits = false;  break; }
            int c = nearest(P, lo, hi, (double)P[len] * i / k);
            while (c > lo && P[c] - P[C.back()] > (uint64_t)cap) c--;
            if (P[c] - P[C.back()] > (uint64_t)cap) fits = false;
            C.push_back(c);
        }
        C.push_back(len);
        const int m = (int)C.size();
        if (!fits || m != k + 1 || (P[len] - P[C[m - 2]] > (uint64_t)cap && len - C[m - 2] > 1)) C = G;
    }
    static int len_of(const Box &b, int axis) { return (axis == 0) ? b.dx : (axis == 1) ? b.dy : b.dz; }
    // what a piece that still holds more than cap cells will cost: counted as if halved along every axis
    static double area_rest(const Boxes &R)
    {
        double a = 0.0;
        for (const Box &r : R) a += 4.0 * ((double)r.dx * r.dy + (double)r.dy * r.dz + (double)r.dz * r.dx);
        return a;
    }
    // the numbers of pieces worth trying for an edge of `len` planes whose pieces would ideally be `e` planes long: from pieces
    // that long (all of cap used, were the cuts exact) to pieces that hold 3/4 of it (shrink: what 3/4 does to this edge)
    static void piece_counts(int len, double e, double shrink, int &k0, int &k1)
    {
        const double r = (double)len / e;
        k0 = std::min(len, std::max(1, (int)std::floor(r)));
        k1 = std::min(len, std::max(k0, (int)std::ceil(r / shrink)));
    }
    // a column along `ax` into boxes of <= cap cells; a plane that holds more goes to `rest`
    void column_cut(const Box &c, int ax, Boxes &B, Boxes &rest) const
    {
        if (c.n <= (uint32_t)cap) { B.push_back(c);  return; }
        std::vector<uint64_t> P;
        std::vector<int> C;
        profile(c, ax, P);
        capped_cuts(P, C);
        for (size_t i = 0; i + 1 < C.size(); i++) {
            const Box x = sub_box(c, ax, C[i], C[i + 1], P[C[i + 1]] - P[C[i]]);
            (x.n <= (uint32_t)cap ? B : rest).push_back(x);
        }
    }
    // a slab into columns along `ay`, each cut along `ax`: the number of columns with the smallest area
    void columns_cut(const Box &s, int ay, int ax, Boxes &B, Boxes &rest) const
    {
        if (s.n <= (uint32_t)cap) { B.push_back(s);  return; }
        std::vector<uint64_t> P;
        std::vector<int> C;
        profile(s, ay, P);
        int k0, k1;
        piece_counts(len_of(s, ay), std::sqrt((double)cap * len_of(s, ay) * len_of(s, ax) / (double)s.n), std::sqrt(0.75), k0, k1);
        Boxes T, R, bestT, bestR;
        double abest = -1.0;
        for (int k = k0; k <= k1; k++) {
            T.clear();  R.clear();
            even_cuts(P, k, C);
            for (size_t i = 0; i + 1 < C.size(); i++) column_cut(sub_box(s, ay, C[i], C[i + 1], P[C[i + 1]] - P[C[i]]), ax, T, R);
            const double a = area(T) + area_rest(R);
            if (abest < 0.0 || a < abest) { abest = a;  bestT.swap(T);  bestR.swap(R); }
        }
        B.insert(B.end(), bestT.begin(), bestT.end());
        rest.insert(rest.end(), bestR.begin(), bestR.end());
    }
    // a node into slabs along `az`: the number of slabs with the smallest area.  Returns that area, what is left over included.
    double slab_cut(const Box &b, int az, int ay, int ax, Boxes &B, Boxes &rest) const
    {
        std::vector<uint64_t> P;
        std::vector<int> C;
        profile(b, az, P);
        int k0, k1;
        piece_counts(len_of(b, az), std::cbrt((double)cap * b.dx * b.dy * b.dz / (double)b.n), std::cbrt(0.75), k0, k1);
        Boxes T, R;
        double abest = -1.0;
        for (int k = k0; k <= k1; k++) {
            T.clear();  R.clear();
            even_cuts(P, k, C);
            for (size_t i = 0; i + 1 < C.size(); i++) columns_cut(sub_box(b, az, C[i], C[i + 1], P[C[i + 1]] - P[C[i]]), ay, ax, T, R);
            const double a = area(T) + area_rest(R);
            if (abest < 0.0 || a < abest) { abest = a;  B.swap(T);  rest.swap(R); }
        }
        return abest;
    }
    bool part(const Box &b, Boxes &B) const
    {
        if (b.n <= (uint32_t)cap) { B.push_back(b);  return true; }
        if (b.dx == 1 && b.dy == 1 && b.dz == 1) return false;       // one root cell with more than cap cells below it
        const int axis = (b.dz >= b.dy && b.dz >= b.dx) ? 2 : (b.dy >= b.dx) ? 1 : 0;
        const int len = len_of(b, axis);
        if ((uint64_t)b.n > (uint64_t)SOC_LB_NODE * (uint64_t)cap) {  // a large node: two nodes, each with a density of its own
            std::vector<uint64_t> P;
            profile(b, axis, P);
            const int c = nearest(P, 1, len - 1, 0.5 * (double)P[len]);
            return part(sub_box(b, axis, 0, c, P[c]), B) && part(sub_box(b, axis, c, len, P[len] - P[c]), B);
        }
        {   // a node with a clump in it -- the cells per root cell of its eight octants differ by more than SOC_LB_SKEW -- is halved: slabs
            // of equal count through a clump and the void around it would be plates
            const int hx = (b.dx + 1) / 2, hy = (b.dy + 1) / 2, hz = (b.dz + 1) / 2;
            uint64_t oct[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
            for (int z = 0; z < b.dz; z++)
                for (int y = 0; y < b.dy; y++) {
                    const uint32_t *row = sub.data() + ((size_t)(b.z0 + z) * NY + (b.y0 + y)) * NX + b.x0;
                    uint64_t *o = oct + ((z >= hz) ? 4 : 0) + ((y >= hy) ? 2 : 0);
                    for (int x = 0; x < hx; x++) o[0] += row[x];
                    for (int x = hx; x < b.dx; x++) o[1] += row[x];
                }
            double lo = 0.0, hi = 0.0;
            uint64_t nlo = 0;                                         // cells in the lower half along `axis`
            for (int k = 0; k < 8; k++) {
                const double v = (double)((k & 1) ? b.dx - hx : hx) * ((k & 2) ? b.dy - hy : hy) * ((k & 4) ? b.dz - hz : hz);
                if (!((k >> axis) & 1)) nlo += oct[k];
                if (v <= 0.0) continue;
                const double rho = (double)oct[k] / v;
                if (hi == 0.0 || rho > hi) hi = rho;
                if (lo == 0.0 || rho < lo) lo = rho;
            }
            if (hi > SOC_LB_SKEW * lo) {
                const int h = (len + 1) / 2;
                return part(sub_box(b, axis, 0, h, nlo), B) && part(sub_box(b, axis, h, len, (uint64_t)b.n - nlo), B);
            }
        }
        // slabs along z, columns along y, boxes along x; a node that is thin against the boxes it will get is tried in all six orders
        static const int ORD[6][3] = { { 2, 1, 0 }, { 2, 0, 1 }, { 1, 2, 0 }, { 1, 0, 2 }, { 0, 2, 1 }, { 0, 1, 2 } };
        const double e = std::cbrt((double)cap * b.dx * b.dy * b.dz / (double)b.n);
        const int nord = ((double)std::min(b.dx, std::min(b.dy, b.dz)) < 3.0 * e) ? 6 : 1;
        Boxes best, bestrest, T, R;
        double abest = -1.0;
        for (int o = 0; o < nord; o++) {
            T.clear();  R.clear();
            const double a = slab_cut(b, ORD[o][0], ORD[o][1], ORD[o][2], T, R);
            bool same = false;                                        // (a piece that is the node itself: no progress)
            for (const Box &r : R) same = same || (r.dx == b.dx && r.dy == b.dy && r.dz == b.dz);
            if (same) continue;
            if (abest < 0.0 || a < abest) { abest = a;  best.swap(T);  bestrest.swap(R); }
        }
        if (abest < 0.0) {                                            // one plane thick where it would have to be cut: halved
            const int h = (len + 1) / 2;
            const Box lo = sub_box(b, axis, 0, h, 0);
            const uint64_t nlo = cells_in(lo.x0, lo.y0, lo.z0, lo.dx, lo.dy, lo.dz);
            return part(sub_box(b, axis, 0, h, nlo), B) && part(sub_box(b, axis, h, len, (uint64_t)b.n - nlo), B);
        }
        B.insert(B.end(), best.begin(), best.end());
        for (const Box &r : bestrest) if (!part(r, B)) return false;
        return true;
    }
    bool slabs(Boxes &B) const
    {
        const uint64_t n = cells_in(0, 0, 0, NX, NY, NZ);
        if (n > 0xffffffffu) return false;
        return part(Box{ 0, 0, 0, NX, NY, NZ, (uint32_t)n }, B);
    }

    // the boxes of the bricks, nothing built yet: the partition with the smaller face area
    bool boxes(int partition, Boxes &B)
    {
        out = SocLBricksHost();
        if (!count()) return false;
        Boxes S;
        if (!tiles(B)) return false;
        out.area_tiles = area(B);  out.n_tiles = (int)B.size();
        if (partition != SOC_LB_TILES && slabs(S)) {
            out.area_slabs = area(S);  out.n_slabs = (int)S.size();
            out.slabs = out.area_slabs < out.area_tiles;
        }
        if (out.slabs) B.swap(S);
        return true;
    }
    bool build(int partition)
    {
        Boxes B;
        if (!boxes(partition, B)) return false;
        out.rbrick.assign((size_t)NX * NY * NZ, -1);
        size_t total = 0;
        for (int l = 0; l < LEVELS; l++) total += (size_t)LCELLS[l];
        out.btree.reserve(total);
        out.bcell.reserve(total);
        for (const Box &b : B) if (!emit(b.x0, b.y0, b.z0, b.dx, b.dy, b.dz, (int)b.n)) return false;
        out.ok = true;
        return true;
    }
};

}  // namespace soc_lb

// Returns false (and out.ok == false) when the hierarchy cannot be cut into such bricks: the caller keeps the
// sweep that reads the hierarchy from global memory.
inline bool soc_lbricks_build(int NX, int NY, int NZ, int LEVELS, const int *LCELLS, const int *OFF, const float *DENS, int cap,
                              SocLBricksHost &out, int partition = SOC_LB_BEST)
{
    soc_lb::Builder B(NX, NY, NZ, LEVELS, LCELLS, OFF, DENS, cap, out);
    const bool ok = B.build(partition);
    if (!ok) out = SocLBricksHost();
    return ok;
}

// Bricks of a single-level (Cartesian) grid, for the sweep of rays on such grids (soc_brick.hip: soc_lbrick_walk<., RAY, ., ., CART>):
// boxes of at most edge^3 root cells, the last box of an axis as short as the grid leaves it (an axis shorter than `edge` is one box).
// The same tables as above with nothing below the root cells: a brick's slots are its cells, x fastest, and hold their densities.
// Returns false for a grid with a cell whose density is not positive: the hierarchy's own walk (the event lanes use it) would read
// such a cell as a link.
inline bool soc_cbricks_build(int NX, int NY, int NZ, const float *DENS, int edge, SocLBricksHost &out)
{
    out = SocLBricksHost();
    if (NX < 1 || NY < 1 || NZ < 1 || edge < 1) return false;
    const size_t cells = (size_t)NX * NY * NZ;
    for (size_t i = 0; i < cells; i++) if (!(DENS[i] > 0.0f)) return false;
    out.rbrick.assign(cells, -1);
    out.btree.resize(cells);
    out.bcell.resize(cells);
    size_t fill = 0;
    for (int z0 = 0; z0 < NZ; z0 += edge)
        for (int y0 = 0; y0 < NY; y0 += edge)
            for (int x0 = 0; x0 < NX; x0 += edge) {
                SocLBrick K;
                K.x0 = x0;  K.y0 = y0;  K.z0 = z0;
                K.bx = (x0 + edge <= NX) ? edge : NX - x0;  K.by = (y0 + edge <= NY) ? edge : NY - y0;  K.bz = (z0 + edge <= NZ) ? edge : NZ - z0;
                K.base = (int)fill;
                K.nslot = K.bx * K.by * K.bz;
                const int id = (int)out.bricks.size();
                for (int z = z0; z < z0 + K.bz; z++)
                    for (int y = y0; y < y0 + K.by; y++)
                        for (int x = x0; x < x0 + K.bx; x++) {
                            const size_t r = ((size_t)z * NY + y) * NX + x;
                            out.rbrick[r] = id;
                            out.bcell[fill] = (int)r;
                            out.btree[fill] = DENS[r];
                            fill++;
                        }
                out.bricks.push_back(K);
                if (K.nslot > out.max_slots) out.max_slots = K.nslot;
            }
    out.ok = true;
    return true;
}

#endif  // SOC_LBRICKS_H
