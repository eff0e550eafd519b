// Stand-alone check of the tile layout and lane maps of csrc/pqp_halfsched.h
// (where an entry of a tile sits in LDS, which lane loads and stores which
// piece, how a diagonal tile's fourth quadrant is made from its mirror).
// Built with -fsanitize=address,undefined and run by tests/test_half_layout.py;
// no GPU, no Python loading.  It works on the header's functions only.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
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

constexpr int kLanes = 64;

// The LDS rules the layout was chosen for, as data: an instruction's 64 lanes
// are served in fixed lane groups, one LDS cycle per group when no two lanes of
// the group want different words of one bank; the bank of word w is w mod
// `banks`.  A lane that wants the same word as another is a broadcast.
struct Form {
    const char* name;
    int words;       // words per lane
    int group;       // lanes per group, consecutive: {0..group-1}, {group..}, ...
    int banks;       // bank = word address mod banks
    int max_ways;    // distinct words on one bank within a group that cost nothing
};
static const Form kWriteB64 = {"ds_write_b64", 2, 16, 32, 1};
static const Form kWriteB32 = {"ds_write_b32", 1, 32, 32, 2};  // 2-way is hidden behind the data transfer
static const Form kReadB32 = {"ds_read_b32", 1, 32, 32, 1};
static const Form kReadB64 = {"ds_read_b64", 2, 32, 64, 1};

// one wave-instruction: addr[lane] = first word, or -1 for a lane that is off
static int ways(const Form& f, const std::vector<int>& addr) {
    int worst = 0;
    for (int g0 = 0; g0 < kLanes; g0 += f.group) {
        std::map<int, std::set<int>> on_bank;
        for (int l = g0; l < g0 + f.group; ++l) {
            if (addr[l] < 0) continue;
            for (int w = 0; w < f.words; ++w) on_bank[(addr[l] + w) % f.banks].insert(addr[l] + w);
        }
        for (const auto& b : on_bank)
            if ((int)b.second.size() > worst) worst = (int)b.second.size();
    }
    return worst;
}
static void check_access(const Form& f, const std::vector<int>& addr, const char* what, int a, int b) {
    for (int l = 0; l < kLanes; ++l) {
        if (addr[l] < 0) continue;
        CHECK(addr[l] >= 0 && addr[l] + f.words <= kTileWords, "%s %d/%d lane %d: word %d outside the tile", what, a, b,
              l, addr[l]);
        if (f.words == 2) CHECK(addr[l] % 2 == 0, "%s %d/%d lane %d: word %d is not 8-byte aligned", what, a, b, l, addr[l]);
        for (int w = 0; w < f.words; ++w)
            CHECK((addr[l] + w) % kTileStride < kTile, "%s %d/%d lane %d: touches padding word %d", what, a, b, l,
                  (addr[l] + w) % kTileStride);
    }
    const int n = ways(f, addr);
    CHECK(n <= f.max_ways, "%s %d/%d: %d-way bank conflict as %s", what, a, b, n, f.name);
}

// what one load instruction of a wave reads from HBM: whole 128-byte runs (32
// rows) of each k it touches
static void check_runs(const std::vector<std::pair<int, int>>& pieces, const char* what, int j) {
    std::map<int, std::set<int>> rows_of_k;
    for (const auto& p : pieces)
        for (int m = 0; m < kPieceRows; ++m) rows_of_k[p.second].insert(p.first + m);
    for (const auto& kv : rows_of_k) {
        for (int r0 = 0; r0 < kTile; r0 += 32) {
            int n = 0;
            for (int r = r0; r < r0 + 32; ++r) n += (int)kv.second.count(r);
            CHECK(n == 0 || n == 32, "%s load %d: k %d reads %d of rows %d..%d", what, j, kv.first, n, r0, r0 + 31);
        }
    }
}

int main() {
    CHECK(kTileStride % 2 == 0 && kTileStride >= kTile, "stride %d", kTileStride);
    CHECK(kTileWords == kTile * kTileStride, "tile words");
    CHECK(kHalfLoads * kLanes * kPieceRows == kTile * kHalfCols, "a half is %d loads per lane", kHalfLoads);
    CHECK(kQuadLoads * kLanes * kPieceRows == kHalfCols * kHalfCols, "a quadrant is %d loads per lane", kQuadLoads);
    // tiles start on 8 bytes: 2 x 1024 words of y, then whole tiles
    CHECK((2 * 1024) % 2 == 0 && kTileWords % 2 == 0, "tile base alignment");
    CHECK(((size_t)2 * 1024 + (size_t)kSlots * kTileWords + kFlagWords) * 4 <= 160 * 1024, "LDS budget");

    // --- a pair's tile: the lower wave stores half 1, the higher one half 2 ---
    std::vector<int> seen(kTile * kTile, 0);
    for (int halves = 1; halves <= 2; ++halves) {
        const int c0 = first_half_col(halves);
        for (int j = 0; j < kHalfLoads; ++j) {
            std::vector<std::pair<int, int>> pieces;
            std::vector<int> lo(kLanes), hi(kLanes);
            for (int l = 0; l < kLanes; ++l) {
                const int r = piece_row(l), k = c0 + piece_col(l) + 4 * j;
                CHECK(r >= 0 && r + kPieceRows <= kTile && r % kPieceRows == 0, "lane %d: piece row %d", l, r);
                CHECK(k >= c0 && k < c0 + kHalfCols, "lane %d load %d: k %d outside half %d", l, j, k, halves);
                pieces.push_back({r, k});
                for (int m = 0; m < kPieceRows; ++m) ++seen[(r + m) * kTile + k];
                lo[l] = tile_word(r, k);      // rows r, r + 1
                hi[l] = tile_word(r + 2, k);  // rows r + 2, r + 3
                CHECK(hi[l] == lo[l] + 2, "lane %d: a piece is not 4 consecutive words", l);
            }
            check_runs(pieces, "half", j);
            check_access(kWriteB64, lo, "half store, rows r..r+1", halves, j);
            check_access(kWriteB64, hi, "half store, rows r+2..r+3", halves, j);
        }
    }
    for (int i = 0; i < kTile * kTile; ++i)
        CHECK(seen[i] == 1, "pair tile: entry (%d, %d) stored %d times", i / kTile, i % kTile, seen[i]);

    // --- a diagonal tile: half 1, the quadrant below the diagonal, the mirror stores ---
    std::vector<int> dseen(kTile * kTile, 0);
    std::vector<int> loaded(kTile * kTile, 0);   // entries that come from HBM
    int loads = 0;
    for (int j = 0; j < kHalfLoads; ++j, ++loads)
        for (int l = 0; l < kLanes; ++l)
            for (int m = 0; m < kPieceRows; ++m) {
                ++dseen[(piece_row(l) + m) * kTile + piece_col(l) + 4 * j];
                ++loaded[(piece_row(l) + m) * kTile + piece_col(l) + 4 * j];
            }
    for (int j = 0; j < kQuadLoads; ++j, ++loads) {
        std::vector<std::pair<int, int>> pieces;
        std::vector<int> lo(kLanes), hi(kLanes);
        for (int l = 0; l < kLanes; ++l) {
            const int r = quad_row(l), k = quad_col(l) + 8 * j;
            CHECK(r >= kHalfCols && r + kPieceRows <= kTile && k >= kHalfCols && k < kTile, "lane %d: quadrant piece (%d, %d)",
                  l, r, k);
            pieces.push_back({r, k});
            for (int m = 0; m < kPieceRows; ++m) {
                ++dseen[(r + m) * kTile + k];
                ++loaded[(r + m) * kTile + k];
            }
            lo[l] = tile_word(r, k);
            hi[l] = tile_word(r + 2, k);
        }
        check_runs(pieces, "quadrant", j);
        check_access(kWriteB64, lo, "quadrant store, rows r..r+1", 3, j);
        check_access(kWriteB64, hi, "quadrant store, rows r+2..r+3", 3, j);
    }
    CHECK(loads == 12, "a diagonal wave issues %d loads", loads);
    int mirror_lanes = 0;
    for (int l = 0; l < kLanes; ++l) mirror_lanes += mirrors(l);
    CHECK(mirror_lanes == kLanes / 2, "%d lanes mirror", mirror_lanes);
    for (int j = 0; j < kHalfLoads; ++j)
        for (int m = 0; m < kPieceRows; ++m) {
            std::vector<int> addr(kLanes, -1);
            for (int l = 0; l < kLanes; ++l) {
                if (!mirrors(l)) continue;
                // the lane holds Q(r, c) of the first half and stores it at (row c, k r)
                const int r = piece_row(l) + m, c = piece_col(l) + 4 * j;
                CHECK(r >= kHalfCols && c < kHalfCols, "lane %d mirrors (%d, %d), not below the diagonal's quadrant", l, r, c);
                CHECK(loaded[r * kTile + c] == 1, "mirror source (%d, %d) is not loaded", r, c);
                ++dseen[c * kTile + r];  // entry (row c, k r): its transpose is the source (r, c)
                CHECK(loaded[c * kTile + r] == 0, "entry (%d, %d) is loaded and mirrored", c, r);
                addr[l] = tile_word(c, r);
            }
            check_access(kWriteB32, addr, "mirror store", j, m);
        }
    for (int i = 0; i < kTile * kTile; ++i)
        CHECK(dseen[i] == 1, "diagonal tile: entry (%d, %d) stored %d times", i / kTile, i % kTile, dseen[i]);
    int from_hbm = 0;
    for (int i = 0; i < kTile * kTile; ++i) from_hbm += loaded[i];
    CHECK(4 * from_hbm == 3 * kTile * kTile, "a diagonal tile reads %d entries from HBM", from_hbm);

    // --- the reads: 64 k per wave and step ---
    std::vector<int> rseen(kTile * kTile, 0), tseen(kTile * kTile, 0);
    for (int k = 0; k < kTile; ++k) {  // straight: lane = row i
        std::vector<int> addr(kLanes);
        for (int l = 0; l < kLanes; ++l) {
            addr[l] = tile_word(l, k);
            ++rseen[l * kTile + k];
        }
        check_access(kReadB32, addr, "straight read", k, 0);
    }
    for (int i = 0; i < kTile; i += 2) {  // transposed: lane = k, entries i and i + 1
        std::vector<int> addr(kLanes);
        for (int l = 0; l < kLanes; ++l) {
            addr[l] = tile_word(i, l);
            CHECK(tile_word(i + 1, l) == addr[l] + 1, "transposed pair (%d, %d) is not consecutive", i, l);
            ++tseen[i * kTile + l];
            ++tseen[(i + 1) * kTile + l];
        }
        check_access(kReadB64, addr, "transposed read", i, 0);
    }
    for (int i = 0; i < kTile * kTile; ++i)
        CHECK(rseen[i] == 1 && tseen[i] == 1, "entry %d read %d / %d times", i, rseen[i], tseen[i]);

    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("layout ok\n");
    return 0;
}
