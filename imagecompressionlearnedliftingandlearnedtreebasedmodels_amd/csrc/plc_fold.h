// Host-side rule of the Winograd tree pair (k_plc_wino, conv_f16x3.hip): does one workgroup per pixel tile that loops over the
// tile's channel blocks ("folded") beat one workgroup per (tile, channel block)?  Plain C++ with no HIP in it, so that a CPU test
// can compile it (tests/test_plc_fold_rule.py).
#pragma once
#include <cstdint>

namespace lldwt {

// What a later pass of a folded workgroup saves, in thousandths of a single-block workgroup's time T: it has no parent patch, no
// |max|, no im2col and no chunk-0 rows, and its workgroup does not start again.  Measured at the bench shape (profiles/README.md,
// round 11).
constexpr int PLC_FOLD_SAVING_PERMILLE = 90;

// n = pixel tiles x images of the launch, cus = compute units (one workgroup of this kernel fills a CU), nocb = channel blocks per
// tile.  The launch runs in rounds of `cus` workgroups.  Unfolded: ceil(nocb n / cus) rounds of T.  Folded: ceil(n / cus) rounds of
// nocb T - (nocb - 1) s.  Folding halves the workgroups, so a launch of a few rounds can lose more to its last, partly filled round
// than the passes save: 384 tiles x 2 blocks on 256 CUs are 3 rounds of T unfolded and 2 rounds of 2T - s folded.
inline bool plc_fold_pays(int64_t n, int cus, int nocb) {
    if (nocb < 2 || n < 1 || cus < 1) return false;
    const int64_t rounds_folded = (n + cus - 1) / cus, rounds_unfolded = (n * nocb + cus - 1) / cus;
    return rounds_folded * ((int64_t)nocb * 1000 - (int64_t)(nocb - 1) * PLC_FOLD_SAVING_PERMILLE) < rounds_unfolded * 1000;
}

}  // namespace lldwt
