// pqp_halfsched.h -- the skewed wave schedule of k_batch_half (pqp_kernels.hip):
// the batched update at n_dual 1024 with every 64 x 64 tile of a bit-symmetric
// Qd read from HBM once for the tile and its mirror.
//
// One workgroup of 16 waves owns one problem; wave I owns rows 64 I .. 64 I + 63
// (one row per lane).  Time runs in steps T = 0 .. 16 C + 14 for C updates.  At
// step T wave I is at s = T - I; for 0 <= s < 16 C it sums k-block K = s mod 16
// of update h = s div 16.  Every wave meets K = 0 .. 15 in order (the per-row
// sum order of the other kernels), and wave I is at k-block K exactly when wave
// K is at k-block I (I + K = T mod 16): tile (I, K) and its mirror (K, I) are
// consumed in the same step, from one copy in LDS that the two waves load half
// each.  Wave I reads it straight, wave K transposed.  A diagonal tile (I, I) is
// symmetric in itself: its wave loads three quarters of it and writes the
// fourth from the mirror quadrant it holds.
//
// These functions are the schedule: the kernel calls them and restates none of
// the arithmetic, and tests/halfsched/halfsched_check.cpp proves the hazards
// on them (every (h, I, K) once, K ascending, pairs agree on slot and halves,
// no slot shared within a step, every y read after its write, no y write under
// a later reader, 136 C tile loads: 16 C diagonal + 120 C pairs).  The flag
// words of the product-first sums (below) ride on the same hazards.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PQP_HS_HD __host__ __device__ inline
#else
#define PQP_HS_HD inline
#endif

namespace pqp {
namespace hs {

constexpr int kWaves = 16;       // waves per workgroup = 64-row blocks of n_dual 1024
constexpr int kTile = 64;        // tile edge (rows per wave, k per step)
constexpr int kTileStride = 66;  // LDS words between two k of a tile: even, so that a row of k starts on 8 bytes
constexpr int kTileWords = kTile * kTileStride;
constexpr int kSlots = 9;        // tiles in LDS per step: at most 7 pairs + 2 diagonal
constexpr int kHalfCols = 32;    // k columns of a tile in one half

// steps of a launch of C updates
PQP_HS_HD int steps(int C) { return C > 0 ? kWaves * C + kWaves - 1 : 0; }

// the wave that consumes this wave's mirror tiles at step T (itself on a
// diagonal tile); defined whether or not either wave is active
PQP_HS_HD int partner(int T, int wave) { return (((T - wave) % kWaves) + kWaves) % kWaves; }

// does `wave` sum a k-block at step T of a launch of C updates
PQP_HS_HD bool active(int T, int wave, int C) {
    const int s = T - wave;
    return s >= 0 && s < kWaves * C;
}
// the update (0-based within the launch) and k-block of an active wave
PQP_HS_HD int update_of(int T, int wave) { return (T - wave) / kWaves; }
PQP_HS_HD int kblock_of(int T, int wave) { return (T - wave) % kWaves; }  // == partner(T, wave)

// Wave I sums k-block K of update h at step 16 h + I + K, which is symmetric in
// I and K: the two waves of a pair are active together, at the same update, in
// the fill and the drain as well.  No tile is ever consumed alone.

// The pair's tile in memory is (rows of the lower wave, k of the higher one):
// element (i, k) at k * ldq + i.  The lower wave reads it straight (its rows
// are the tile's rows), the higher one transposed.
PQP_HS_HD int tile_rows(int T, int wave) {
    const int p = partner(T, wave);
    return wave < p ? wave : p;
}
PQP_HS_HD int tile_cols(int T, int wave) {
    const int p = partner(T, wave);
    return wave < p ? p : wave;
}
PQP_HS_HD bool transposed(int T, int wave) { return wave > partner(T, wave); }
// a self-paired wave: its tile holds its rows' diagonal entries
PQP_HS_HD bool diagonal(int T, int wave) { return partner(T, wave) == wave; }

// Which halves of the tile (bit 0: k columns 0..31, bit 1: 32..63) this wave
// loads for step T: the lower wave of a pair the first, the higher one the
// second, a self-paired wave both -- of the second only the quadrant below the
// diagonal (rows 32..63, quad_*() below): 3/4 of the tile's bytes.
PQP_HS_HD int load_halves(int T, int wave, int C) {
    if (!active(T, wave, C)) return 0;
    const int p = partner(T, wave);
    return p == wave ? 3 : (wave < p ? 1 : 2);
}

// first k column of the first (or only) half in a load_halves() mask
PQP_HS_HD int first_half_col(int halves) { return (halves & 1) ? 0 : kHalfCols; }

// The tile in LDS and the lanes' pieces of it.  Entry (i, k) of a tile sits at
// word k * 66 + i of its slot (words 64 and 65 of a row of k are padding that
// nothing reads or writes).
//  - The straight read (lane = i, the lower wave and a diagonal wave) takes
//    word k * 66 + lane: 64 consecutive words per ds_read_b32.
//  - The transposed read (lane = k, the higher wave: Qd(k, i) for Qd(i, k))
//    takes the 8-byte pair i, i + 1 at lane * 66 + i with one ds_read_b64; rows
//    start 66 = 2 mod 64 words apart, so the 32 lanes of a lane group cover 64
//    banks.
//  - A piece is what one 16-byte load brings: rows r .. r + 3 of one k.  It goes
//    to LDS as two ds_write_b64, which are served in groups of 16 consecutive
//    lanes on 32 banks: lane bits 0-2 and 4 choose the row group, bits 3 and 5
//    the k, so a group of 16 lanes holds 8 adjacent row groups (banks 4 g,
//    4 g + 1 or 4 g + 2, 4 g + 3) at two adjacent k, and the odd k, 66 words on,
//    falls into the banks the even one leaves free.  A half has 8 loads per
//    lane, load j at k piece_col(lane) + 4 j of the half: every load
//    instruction still reads whole k of 256 bytes.
//  - The quadrant of a diagonal tile (rows 32..63, k 32..63) has 4 loads per
//    lane: lane bits 0-2 choose the row group, bits 3-5 the k, load j at k
//    quad_col(lane) + 8 j: whole 128-byte runs, and the same 16-lane groups.
//  - The quadrant above the diagonal (rows 0..31, k 32..63) is never loaded.
//    The lanes whose pieces of the first half lie in rows 32..63 (mirrors())
//    store each value Q(r, c) a second time at (row c, k r), one ds_write_b32
//    each: by the caller's contract these are the bits of Q(c, r).
// tests/halfsched/half_layout_check.cpp checks coverage, alignment and bank
// conflicts on these functions.
constexpr int kPieceRows = 4;   // rows of one 16-byte load
constexpr int kHalfLoads = 8;   // loads per lane for one half
constexpr int kQuadLoads = 4;   // loads per lane for a diagonal tile's quadrant
PQP_HS_HD int tile_word(int i, int k) { return k * kTileStride + i; }
PQP_HS_HD int piece_row(int lane) { return kPieceRows * ((lane & 7) | ((lane >> 1) & 8)); }
PQP_HS_HD int piece_col(int lane) { return ((lane >> 3) & 1) | ((lane >> 4) & 2); }  // + 4 j within the half
PQP_HS_HD int quad_row(int lane) { return kHalfCols + kPieceRows * (lane & 7); }
PQP_HS_HD int quad_col(int lane) { return kHalfCols + (lane >> 3); }  // + 8 j
PQP_HS_HD bool mirrors(int lane) { return piece_row(lane) >= kHalfCols; }

// LDS slot (0 .. kSlots - 1) of the pair's tile at step T.  With t = T mod 16
// the pairs have I + K = t (lower wave 0 .. t/2) or t + 16 (lower wave t + 1 ..
// (t + 16)/2): the first group takes its lower wave's number, the second
// follows on.
PQP_HS_HD int slot(int T, int wave) {
    const int t = ((T % kWaves) + kWaves) % kWaves;
    const int p = partner(T, wave);
    const int lo = wave < p ? wave : p;
    return (wave + p == t) ? lo : lo - (t + 1) / 2;
}

// y ping-pong: update h reads the iterate from buffer h & 1 and writes the
// next one into the other
PQP_HS_HD int y_read_buf(int h) { return h & 1; }
PQP_HS_HD int y_write_buf(int h) { return (h + 1) & 1; }

// an active wave at its last k-block runs the update's epilogue in that step
PQP_HS_HD bool last_kblock(int T, int wave) { return kblock_of(T, wave) == kWaves - 1; }

// Flag words of the product-first sums (k_batch_half<true>): an off-diagonal
// tile is summed in the cheaper form only while all of its q are finite and
// every y of the k-block is finite with its sign bit clear; a set flag sends
// the wave to the lean form for that step.
//  - One word per slot and half, written by the wave that loads the half, with
//    the half itself, before the step's first barrier, and read after it by
//    the pair's two waves: the tile's own hazard (no slot shared in a step).
//  - One word per y buffer and k-block: wave I alone writes k-block I of the
//    iterate (from Y0 before the first barrier, from its epilogue afterwards)
//    and the block's flag in the same place.  The flag has the writer, the
//    step and the readers of the y block it describes, so the y checks of
//    tests/halfsched/halfsched_check.cpp (every read a step after its write,
//    no write under a later reader) hold for it as they stand.
constexpr int kFlagWords = 2 * kSlots + 2 * kWaves;
PQP_HS_HD int tile_flag(int T, int wave, int half) { return 2 * slot(T, wave) + half; }  // half: 0 or 1
PQP_HS_HD int y_flag(int buf, int kblock) { return 2 * kSlots + buf * kWaves + kblock; }
// the half a load_halves() mask of one half names
PQP_HS_HD int half_of(int halves) { return halves >> 1; }
// y (as its bits) is not finite, or has its sign bit set (-0 too)
PQP_HS_HD bool y_dirty(unsigned bits) { return !(bits < 0x7f800000u); }
// sticky fold over a half-tile's q, from s = +0: NaN from the first inf or NaN
// q on (q * 0), +0 before it; q_dirty(s) tests the fold
PQP_HS_HD float q_fold(float s, float q) { return __builtin_fmaf(q, 0.0f, s); }
PQP_HS_HD bool q_dirty(float s) { return s != s; }

}  // namespace hs
}  // namespace pqp
