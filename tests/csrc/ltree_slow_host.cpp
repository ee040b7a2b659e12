// ltree_slow_host.cpp -- stand-alone host check of the slow-step test of soc_lt_aim (soc_ltree.h, double form) after it became straight-line
// code (three-way minima, "the smallest fractional part is zero", a select on `sib`): the outcome of soc_lt_aim against the expression it
// replaced, kept here as the statement of record, not in the product.  Equality everywhere, no tolerance.  Built with
// -fsanitize=address,undefined and run as a program (tests/test_ltree_slow_host.py).
//
// soc_lt_aim returns SOC_LT_SLOW exactly when its `slow` holds (go = !slow & ..., and SLOW is the first alternative of a step that does not go),
// so A.r == SOC_LT_SLOW is the predicate under test.  Covered: every level L 1..7 of every Lmax <= 7 for two root-grid sizes (kexp), both values
// of `sib` (counted, both must occur for every L), and per axis the bit-pattern neighbourhoods of +0 and -0, the denormals, the smallest normal
// number, the cell faces 0..3 +- 4 ulp, the two bounds 2^(kexp+1) and 2^(kexp+L) +- 4 ulp, interior points, and the negatives of all of them --
// each of these on one axis with every pair of a smaller companion set on the other two, for every choice of the axis -- then seeded random
// positions: uniform over the octet and its surroundings, and random bit patterns of every exponent below 2^20 (no NaN, no infinity).
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>
#include "soc_ltree.h"

// the parent's expression, as it stood in soc_lt_aim
static bool old_slow(float px, float py, float pz, int L, int Lmax, int kexp)
{
    const int D = Lmax - L;
    const float sc = soc_lt_pow2(D);
    const int Jx = (int)soc_floorf(px * sc), Jy = (int)soc_floorf(py * sc), Jz = (int)soc_floorf(pz * sc);
    const bool deep = (L > 0), place = false;
    const bool sib = deep & !place & ((((unsigned)(Jx | Jy | Jz)) >> (D + 1)) == 0u);
    const float mabs = soc_fminf(soc_fabsf(px), soc_fminf(soc_fabsf(py), soc_fabsf(pz)));
    const float mmin = soc_fminf(px, soc_fminf(py, pz));
    const bool onface = (px == soc_floorf(px)) || (py == soc_floorf(py)) || (pz == soc_floorf(pz));
    return deep & !place & (sib ? !(mmin >= soc_lt_pow2(kexp + 1)) : (!(mabs >= soc_lt_pow2(kexp + L)) | onface));
}

static bool is_sib(float px, float py, float pz, int L, int Lmax)
{
    const int D = Lmax - L;
    const float sc = soc_lt_pow2(D);
    const int Jx = (int)soc_floorf(px * sc), Jy = (int)soc_floorf(py * sc), Jz = (int)soc_floorf(pz * sc);
    return (((unsigned)(Jx | Jy | Jz)) >> (D + 1)) == 0u;
}

static long n_checked = 0, n_sib = 0, n_far = 0, n_slow = 0;

static bool check(float px, float py, float pz, int L, int Lmax, int kexp)
{
    SocLBrick K;  K.x0 = 2;  K.y0 = 3;  K.z0 = 1;  K.bx = 4;  K.by = 3;  K.bz = 5;  K.base = 0;  K.nslot = 1 << 20;
    const int cx = (3 << L) | 5, cy = (4 << L) | 2, cz = (2 << L) | 7, obase = 4096 + 8 * L;
    SocLtAim A;
    soc_lt_aim(K, 1 << (kexp + 29), 1 << (kexp + 29), 1 << (kexp + 29), Lmax, kexp, SOC_LTM_STEP, px, py, pz, L, cx, cy, cz, obase, A);
    const bool got = (A.r == SOC_LT_SLOW), want = old_slow(px, py, pz, L, Lmax, kexp);
    n_checked++;
    if (is_sib(px, py, pz, L, Lmax)) n_sib++; else n_far++;
    n_slow += want ? 1 : 0;
    if (got != want) {
        std::printf("slow: Lmax %d L %d kexp %d pos %a %a %a (%08x %08x %08x): %d, expected %d\n", Lmax, L, kexp, (double)px, (double)py, (double)pz,
                    soc_f2u(px), soc_f2u(py), soc_f2u(pz), (int)got, (int)want);
        return false;
    }
    return true;
}

// v and the four floats on either side of it, by bit pattern (of a positive v; a pattern below zero wraps to the negative side: -0 and the
// negative denormals, which is what the neighbourhood of +0 has there)
static void around(std::vector<float> &out, float v)
{
    const uint32_t u = soc_f2u(v);
    for (int d = -4; d <= 4; d++) {
        const int64_t w = (int64_t)u + d;
        out.push_back((w >= 0) ? soc_u2f((uint32_t)w) : soc_u2f(0x80000000u + (uint32_t)(-w - 1)));
    }
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;  rng_state ^= rng_state >> 7;  rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}
// a random finite float of any exponent below 2^20, either sign
static float rnd_bits()
{
    uint32_t u = rnd();
    const uint32_t ex = (u >> 23) & 0xffu;
    if (ex > 146u) u = (u & 0x807fffffu) | ((ex % 147u) << 23);
    return soc_u2f(u);
}
static float rnd_uniform(float lo, float hi) { return lo + (hi - lo) * ((float)(rnd() >> 8) * (1.0f / 16777216.0f)); }

int main()
{
    for (int k = 7; k <= 10; k += 3) {
        const int kexp = k - 30;
        for (int Lmax = 1; Lmax <= 7; Lmax++)
            for (int L = 1; L <= Lmax; L++) {
                const long sib0 = n_sib, far0 = n_far;
                std::vector<float> pos;
                around(pos, 0.0f);                                   // +0, the smallest denormals, -0 and the negative denormals
                around(pos, soc_u2f(0x00800000u));                   // the smallest normal number and the largest denormals
                for (int f = 1; f <= 3; f++) around(pos, (float)f);  // the faces (0 came first)
                around(pos, soc_lt_pow2(kexp + 1));                  // the two bounds
                around(pos, soc_lt_pow2(kexp + L));
                pos.push_back(0.37f);  pos.push_back(1.62f);  pos.push_back(2.5f);  pos.push_back(3.75f);
                const size_t npos = pos.size();
                for (size_t i = 0; i < npos; i++) pos.push_back(-pos[i]);
                const float comp[] = { 0.37f, 1.62f, 2.5f, -0.3f, 1.0f, 3.0f, 0.0f, -0.0f, soc_u2f(3u), soc_lt_pow2(kexp + L), soc_lt_pow2(kexp + 1),
                                       soc_u2f(soc_f2u(soc_lt_pow2(kexp + L)) - 1u), soc_u2f(soc_f2u(soc_lt_pow2(kexp + 1)) - 1u), -soc_lt_pow2(kexp + 1) };
                const int ncomp = (int)(sizeof(comp) / sizeof(comp[0]));
                for (size_t i = 0; i < pos.size(); i++)
                    for (int a = 0; a < ncomp; a++)
                        for (int b = 0; b < ncomp; b++) {
                            if (!check(pos[i], comp[a], comp[b], L, Lmax, kexp)) return 1;
                            if (!check(comp[a], pos[i], comp[b], L, Lmax, kexp)) return 1;
                            if (!check(comp[a], comp[b], pos[i], L, Lmax, kexp)) return 1;
                        }
                if (n_sib == sib0 || n_far == far0) { std::printf("Lmax %d L %d: one value of sib did not occur\n", Lmax, L);  return 1; }
                // seeded random positions: the octet and its surroundings; one axis close to a face; any finite bit pattern
                for (int n = 0; n < 30000; n++) {
                    if (!check(rnd_uniform(-1.0f, 3.0f), rnd_uniform(-1.0f, 3.0f), rnd_uniform(-1.0f, 3.0f), L, Lmax, kexp)) return 1;
                    if (!check(rnd_uniform(0.0f, 2.0f), rnd_uniform(0.0f, 2.0f), rnd_uniform(0.0f, 2.0f), L, Lmax, kexp)) return 1;
                    const float face = (float)(rnd() % 4u);
                    const float near = soc_u2f(soc_f2u(face + 1.0f) + (rnd() % 9u) - 4u) - 1.0f;      // exact: within 4 ulp(1) of the face
                    if (!check(rnd_uniform(0.0f, 2.0f), near, rnd_uniform(-1.0f, 3.0f), L, Lmax, kexp)) return 1;
                    if (!check(rnd_bits(), rnd_bits(), rnd_bits(), L, Lmax, kexp)) return 1;
                    if (!check(rnd_uniform(0.0f, 2.0f), rnd_bits(), rnd_uniform(0.0f, 2.0f), L, Lmax, kexp)) return 1;
                }
            }
    }
    std::printf("ltree slow ok: %ld positions (%ld sibling, %ld not), %ld slow\n", n_checked, n_sib, n_far, n_slow);
    return 0;
}
