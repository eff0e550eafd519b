// Stand-alone check of the product-first sums of k_batch_half (csrc/
// pqp_kernels.hip, half_tile_sum_pf) against the lean form (lean1), on a host
// model of the two, and of the flag predicates of csrc/pqp_halfsched.h that
// decide which form a wave takes.  Built with -ffp-contract=off and host-side
// sanitizers and run by tests/test_half_pf_forms.py; no GPU, no Python loading.
//
// The claim: while every q is finite and every y finite with its sign bit
// clear, both accumulators of the two forms agree bit for bit after every term,
// whichever sign v_max_f32 gives a zero result.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pqp_halfsched.h"

using namespace pqp::hs;

static int g_fail = 0;
static long long g_terms = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            std::printf("FAIL %s: ", #cond);      \
            std::printf(__VA_ARGS__);             \
            std::printf("\n");                    \
            if (++g_fail > 20) std::exit(1);      \
        }                                         \
    } while (0)

static uint32_t bits(float x) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    return u;
}
static float from_bits(uint32_t u) {
    float x;
    std::memcpy(&x, &u, 4);
    return x;
}

// lean1 of pqp_kernels.hip, word for word
static void lean1(float& ap, float& an, float q, float y) {
    const float z = 0.0f * y;
    const float p = q * y;
    ap += (q < 0.0f) ? z : p;
    an += (q > 0.0f) ? z : -p;
}

// v_max_f32 x, 0: the larger operand, the other one for a NaN x.  Of two zeros
// the hardware may return either; the model gives every zero result the sign
// the caller asks for (more than the hardware can do: a negative x gives +0).
static float vmax0(float x, bool zero_negative) {
    if (x > 0.0f) return x;
    return zero_negative ? -0.0f : 0.0f;
}
// one term of half_tile_sum_pf; zs: bit 0 the den side's zero sign, bit 1 the num side's
static void pf1(float& ap, float& an, float q, float y, int zs) {
    const float p = q * y;
    ap += vmax0(p, zs & 1);
    an += vmax0(-p, (zs >> 1) & 1);
}

// the signs of zero results along a chain: modes 0..3 the same for every term, 4 and 5 changing from term to term
constexpr int kModes = 6;
static int zero_signs(int mode, int term) { return mode < 4 ? mode : (mode == 4 ? term & 3 : (3 * term + 1) & 3); }

struct Term {
    float q, y;
};

// both forms along one chain from +0, compared after every term
static void chain(const std::vector<Term>& t, const char* what) {
    for (int mode = 0; mode < kModes; ++mode) {
        float lp = 0.0f, ln = 0.0f, fp = 0.0f, fn = 0.0f;
        for (size_t i = 0; i < t.size(); ++i) {
            lean1(lp, ln, t[i].q, t[i].y);
            pf1(fp, fn, t[i].q, t[i].y, zero_signs(mode, (int)i));
            ++g_terms;
            CHECK(bits(lp) == bits(fp) && bits(ln) == bits(fn),
                  "%s, mode %d, term %zu of %zu (q %08x y %08x): den %08x / %08x, num %08x / %08x", what, mode, i,
                  t.size(), bits(t[i].q), bits(t[i].y), bits(lp), bits(fp), bits(ln), bits(fn));
            CHECK(bits(lp) != 0x80000000u && bits(ln) != 0x80000000u && lp == lp && ln == ln,
                  "%s: a sum reached -0 or NaN (%08x, %08x)", what, bits(lp), bits(ln));
        }
    }
}

int main() {
    const float dmin = from_bits(0x00000001u), dmax = from_bits(0x007fffffu);
    // every q: special finite floats of both signs and a few ordinary values
    std::vector<float> Q = {0.0f, -0.0f, dmin, -dmin, dmax, -dmax, FLT_MIN, -FLT_MIN, 1.0f, -1.0f,
                            FLT_MAX, -FLT_MAX, 0.3f, -0.3f, 7.25f, -1234.5f, 3.0e-20f, -2.0e19f, 1.5e38f, -1.5e38f};
    // every y: the non-negative finite ones
    std::vector<float> Y = {0.0f, dmin, dmax, FLT_MIN, 1.0f, FLT_MAX, 0.3f, 1000.0f, 2.5e-21f, 3.0e38f, 1.9999999f};
    std::vector<Term> all;
    for (float q : Q)
        for (float y : Y) all.push_back({q, y});
    // single terms and every ordered pair of terms
    for (const Term& a : all) chain({a}, "one term");
    for (const Term& a : all)
        for (const Term& b : all) chain({a, b}, "two terms");
    // chains of a few terms whose products (or sums) overflow to +-inf, with
    // zeros, denormals and ordinary terms before and after the overflow
    const std::vector<Term> ov = {{FLT_MAX, FLT_MAX}, {-FLT_MAX, FLT_MAX}, {FLT_MAX, 2.0f},  {-FLT_MAX, 2.0f},
                                  {1.0f, FLT_MAX},    {-1.0f, FLT_MAX},    {1.5e38f, 3.0f},  {-1.5e38f, 3.0f},
                                  {0.0f, 1.0f},       {-0.0f, FLT_MAX},    {dmin, dmin},     {-dmin, dmax},
                                  {0.3f, 1000.0f},    {-0.3f, 1000.0f}};
    for (const Term& a : ov)
        for (const Term& b : ov)
            for (const Term& c : ov) {
                chain({a, b, c}, "overflow chain of 3");
                for (const Term& d : ov) chain({a, b, c, d}, "overflow chain of 4");
            }
    // a tile's worth of terms (64 k) drawn from the tables
    uint32_t lcg = 12345u;
    auto next = [&](size_t n) {
        lcg = lcg * 1664525u + 1013904223u;
        return (size_t)((lcg >> 8) % n);
    };
    for (int r = 0; r < 2000; ++r) {
        std::vector<Term> t(64);
        for (Term& x : t) x = {Q[next(Q.size())], Y[next(Y.size())]};
        chain(t, "64 terms");
    }

    // the flag predicates.  y: finite with the sign bit clear passes, -0, every
    // negative, +-inf and NaNs of both signs do not
    for (float y : Y) CHECK(!y_dirty(bits(y)), "y %08x taken as dirty", bits(y));
    const uint32_t bad_y[] = {0x80000000u, 0x80000001u, 0xbf800000u, 0xff7fffffu, 0x7f800000u, 0xff800000u,
                              0x7fc00000u, 0xffc00000u, 0x7f800001u, 0x7fc00123u, 0xffffffffu};
    for (uint32_t u : bad_y) CHECK(y_dirty(u), "y %08x taken as clean", u);
    // q: a half-tile's fold (32 values per lane) stays +0 over finite q in any
    // order and is dirty from one inf or NaN at any position on
    {
        float s = 0.0f;
        for (int rep = 0; rep < 2; ++rep)
            for (float q : Q) s = q_fold(s, q);
        CHECK(!q_dirty(s) && bits(s) == 0u, "finite q folded to %08x", bits(s));
        s = 0.0f;
        for (size_t i = Q.size(); i-- > 0;) s = q_fold(s, Q[i]);
        CHECK(!q_dirty(s) && bits(s) == 0u, "finite q (reversed) folded to %08x", bits(s));
    }
    const uint32_t bad_q[] = {0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0x7fc00123u};
    for (uint32_t u : bad_q)
        for (int pos = 0; pos < 32; ++pos) {
            float s = 0.0f;
            for (int i = 0; i < 32; ++i) s = q_fold(s, i == pos ? from_bits(u) : Q[(size_t)i % Q.size()]);
            CHECK(q_dirty(s), "q %08x at %d of 32 folded clean", u, pos);
        }
    // the flags are needed: outside the conditions the two forms do differ
    // (a NaN q or y goes through v_max_f32 as 0, a negative y swaps the sides)
    {
        const Term outside[] = {{1.0f, INFINITY}, {1.0f, -1.0f}, {INFINITY, 0.0f}, {NAN, 1.0f}};
        for (const Term& t : outside) {
            float lp = 0.0f, ln = 0.0f, fp = 0.0f, fn = 0.0f;
            lean1(lp, ln, t.q, t.y);
            pf1(fp, fn, t.q, t.y, 0);
            CHECK(bits(lp) != bits(fp) || bits(ln) != bits(fn), "q %08x y %08x: the forms agree outside the conditions",
                  bits(t.q), bits(t.y));
            CHECK(y_dirty(bits(t.y)) || q_dirty(q_fold(0.0f, t.q)), "q %08x y %08x passes both predicates", bits(t.q),
                  bits(t.y));
        }
    }
    // the flag words fit behind the tiles and name distinct words
    {
        std::vector<int> seen(kFlagWords, 0);
        for (int T = 0; T < kWaves; ++T)
            for (int I = 0; I < kWaves; ++I)
                for (int h = 0; h < 2; ++h) {
                    const int w = tile_flag(T, I, h);
                    CHECK(w >= 0 && w < 2 * kSlots && w == 2 * slot(T, I) + h, "tile_flag(%d, %d, %d) = %d", T, I, h,
                          w);
                    seen[w] = 1;
                }
        for (int b = 0; b < 2; ++b)
            for (int K = 0; K < kWaves; ++K) {
                const int w = y_flag(b, K);
                CHECK(w >= 2 * kSlots && w < kFlagWords && !(seen[w] & 2), "y_flag(%d, %d) = %d", b, K, w);
                seen[w] |= 2;
            }
        for (int w = 0; w < kFlagWords; ++w) CHECK(seen[w] == (w < 2 * kSlots ? 1 : 2), "flag word %d", w);
        CHECK(half_of(1) == 0 && half_of(2) == 1, "half_of");
        CHECK(((size_t)2 * 1024 + (size_t)kSlots * kTileWords + kFlagWords) * 4 <= 160 * 1024, "LDS budget");
    }
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("forms ok (%lld terms)\n", g_terms);
    return 0;
}
