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
// each.  Wave I reads it straight, wave K transposed.
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
constexpr int kTileStride = 65;  // LDS words between two k of a tile: straight and transposed reads hit 64 banks
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
// second, a self-paired wave both.
PQP_HS_HD int load_halves(int T, int wave, int C) {
    if (!active(T, wave, C)) return 0;
    const int p = partner(T, wave);
    return p == wave ? 3 : (wave < p ? 1 : 2);
}

// first k column of the first (or only) half in a load_halves() mask
PQP_HS_HD int first_half_col(int halves) { return (halves & 1) ? 0 : kHalfCols; }

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
