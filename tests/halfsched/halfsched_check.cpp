// Stand-alone check of csrc/pqp_halfsched.h (the skewed wave schedule of
// k_batch_half).  Built with -fsanitize=address,undefined and run by
// tests/test_halfsched.py; no GPU, no Python loading.  For each C it walks
// every step of the launch and checks what the kernel relies on.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pqp_halfsched.h"

using namespace pqp::hs;

static int g_fail = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            std::printf("FAIL %s: ", #cond);      \
            std::printf(__VA_ARGS__);             \
            std::printf("\n");                    \
            if (++g_fail > 20) std::exit(1);      \
        }                                         \
    } while (0)

static void check(int C) {
    const int W = kWaves, S = steps(C);
    CHECK(S == 16 * C + 15, "C=%d steps=%d", C, S);
    std::vector<int> visits((size_t)C * W * W, 0);
    std::vector<int> lastK((size_t)C * W, -1);
    // y_h[block] for h = 0..C: the step that writes it (-1: before the first
    // step) and the last step that reads it
    std::vector<int> wstep((size_t)(C + 1) * W, -2), rlast((size_t)(C + 1) * W, -1);
    for (int b = 0; b < W; ++b) wstep[b] = -1;
    long long half_loads = 0;
    for (int T = 0; T < S; ++T) {
        int slot_owner[kSlots];
        for (int s = 0; s < kSlots; ++s) slot_owner[s] = -1;
        for (int I = 0; I < W; ++I) {
            const int p = partner(T, I);
            CHECK(p >= 0 && p < W, "T=%d I=%d partner=%d", T, I, p);
            CHECK(partner(T, p) == I, "T=%d I=%d: partner not symmetric", T, I);
            CHECK(active(T, I, C) == active(T, p, C), "T=%d I=%d: one wave of the pair works alone", T, I);
            const int lh = load_halves(T, I, C);
            half_loads += (lh & 1) + ((lh >> 1) & 1);
            if (!active(T, I, C)) {
                CHECK(lh == 0, "T=%d I=%d: an idle wave loads", T, I);
                continue;
            }
            CHECK(update_of(T, I) == update_of(T, p), "T=%d I=%d: the pair is at two updates", T, I);
            // the pair agrees on the tile, the slot and the two halves
            const int sl = slot(T, I);
            CHECK(sl >= 0 && sl < kSlots, "T=%d I=%d slot=%d", T, I, sl);
            CHECK(sl == slot(T, p), "T=%d I=%d: the pair names two slots", T, I);
            CHECK(tile_rows(T, I) == tile_rows(T, p) && tile_cols(T, I) == tile_cols(T, p), "T=%d I=%d: tile", T, I);
            CHECK(tile_rows(T, I) == (I < p ? I : p) && tile_cols(T, I) == (I < p ? p : I), "T=%d I=%d: tile", T, I);
            if (p == I) {
                CHECK(lh == 3 && active(T, I, C) && !transposed(T, I), "T=%d I=%d: diagonal tile", T, I);
            } else {
                CHECK((lh | load_halves(T, p, C)) == 3 && (lh & load_halves(T, p, C)) == 0 && (lh == 1 || lh == 2),
                      "T=%d I=%d: halves %d and %d", T, I, lh, load_halves(T, p, C));
                CHECK(transposed(T, I) != transposed(T, p), "T=%d I=%d: both read the same way", T, I);
                CHECK(transposed(T, I) == (I == tile_cols(T, I)), "T=%d I=%d: transposed", T, I);
            }
            // no two pairs of a step share a slot
            const int owner = I < p ? I : p;
            CHECK(slot_owner[sl] == -1 || slot_owner[sl] == owner, "T=%d: slot %d shared by pairs of %d and %d", T,
                  sl, slot_owner[sl], owner);
            slot_owner[sl] = owner;
            const int h = update_of(T, I), K = kblock_of(T, I);
            CHECK(h >= 0 && h < C && K >= 0 && K < W && K == p, "T=%d I=%d h=%d K=%d", T, I, h, K);
            ++visits[((size_t)h * W + I) * W + K];
            CHECK(K == lastK[(size_t)h * W + I] + 1, "T=%d I=%d h=%d: K=%d after %d", T, I, h, K,
                  lastK[(size_t)h * W + I]);
            lastK[(size_t)h * W + I] = K;
            // reads y_h[K] (the sum) and, in the epilogue, y_h[I]; both from buffer y_read_buf(h)
            CHECK(wstep[(size_t)h * W + K] >= -1 && wstep[(size_t)h * W + K] < T, "T=%d I=%d: y_%d[%d] read, written at %d",
                  T, I, h, K, wstep[(size_t)h * W + K]);
            if (rlast[(size_t)h * W + K] < T) rlast[(size_t)h * W + K] = T;
            CHECK(last_kblock(T, I) == (K == W - 1), "T=%d I=%d: last_kblock", T, I);
        }
        // epilogues of this step, after its sums: wave I writes y_{h+1}[I]
        for (int I = 0; I < W; ++I) {
            if (!active(T, I, C) || !last_kblock(T, I)) continue;
            const int h = update_of(T, I);
            CHECK(wstep[(size_t)h * W + I] < T, "T=%d I=%d: epilogue reads y_%d[%d] before its write", T, I, h, I);
            if (rlast[(size_t)h * W + I] < T) rlast[(size_t)h * W + I] = T;
            CHECK(wstep[(size_t)(h + 1) * W + I] == -2, "T=%d I=%d: y_%d[%d] written twice", T, I, h + 1, I);
            wstep[(size_t)(h + 1) * W + I] = T;
            CHECK(y_write_buf(h) == y_read_buf(h + 1) && y_write_buf(h) != y_read_buf(h), "h=%d: y buffers", h);
        }
    }
    // every (h, I, K) exactly once
    for (size_t i = 0; i < visits.size(); ++i) CHECK(visits[i] == 1, "C=%d: visit %zu seen %d times", C, i, visits[i]);
    // a write of y_{h+1}[I] replaces y_{h-1}[I] (same buffer): every read of
    // that one is in a strictly earlier step; reads of y_h[I] in the write's
    // own step go to the other buffer
    for (int h = 1; h + 1 <= C; ++h)
        for (int I = 0; I < W; ++I) {
            CHECK(y_read_buf(h - 1) == y_write_buf(h), "h=%d: ping-pong", h);
            CHECK(rlast[(size_t)(h - 1) * W + I] < wstep[(size_t)(h + 1) * W + I],
                  "C=%d: y_%d[%d] written at %d, y_%d still read at %d", C, h + 1, I, wstep[(size_t)(h + 1) * W + I],
                  h - 1, rlast[(size_t)(h - 1) * W + I]);
        }
    for (int I = 0; I < W; ++I) CHECK(wstep[(size_t)C * W + I] >= 0, "C=%d: y_C[%d] never written", C, I);
    // 16 C diagonal tiles + 120 C pairs.  (The proposal of this schedule
    // expected 136 C + 120, counting 240 fill / drain tiles as consumed alone;
    // the pair check above shows there are none.)
    CHECK(half_loads == 2LL * 136 * C, "C=%d: %lld half-tile loads, want %d", C, half_loads, 2 * 136 * C);
    // nothing is live outside the launch's steps
    for (int I = 0; I < W; ++I)
        CHECK(!active(S, I, C) && !active(-1, I, C) && load_halves(S, I, C) == 0, "C=%d I=%d: active past the end", C,
              I);
}

int main() {
    const int cs[] = {1, 2, 3, 10};
    for (int C : cs) check(C);
    CHECK(steps(0) == 0, "steps(0)");
    CHECK((size_t)kSlots * kTileWords * 4 + 2 * 1024 * 4 <= 160 * 1024, "LDS budget");
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("schedule ok\n");
    return 0;
}
