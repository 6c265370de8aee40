// Host-side rule of the forked eval step (lldwt_lifting_forward_split, lifting.hip): at which level, if at all,
// does the step of the tree-pair layers move the coarse end of the lifting transform -- and what hangs on it: the coarse levels'
// subband MLPs, their quantisation, the coarsest level's context stacks and rates -- to a second stream, beside the level-0 tree
// pair and context MLP?  Plain C++ with no HIP in it, so that a CPU test can compile it (tests/test_lift_split_rule.py).
#pragma once
#include <cstdint>

namespace lldwt {

// The level-i tree pair reads the quantised level i + 1, so with the fork at level k the main stream can run the pairs of the
// levels 0 .. k - 2 before it needs anything from the tail.  k = 1 leaves it nothing to run, and a k above 2 only shortens the
// tail that is hidden: the fork is at level 2 or nowhere.
constexpr int LIFT_SPLIT_LEVEL = 2;

// What the two sides cost, from the kernel traces of the bench step (profiles/r15_overlap.json; 8 x 3 x 512 x 512, 4 levels, 256 CUs):
//   main: the level-0 pair (2.47-2.60 ms) and context MLP (0.77 ms) run at full occupancy: 3.3 ms for 24 x 256 x 256 level-0
//         subband pixels, LIFT_SPLIT_MAIN_PS picoseconds per pixel on one CU's share.
//   tail: a chain of launches too small to fill the chip, 0.95 ms alone.  Each of the 8 launches of a lifting level costs a fixed
//         LIFT_SPLIT_LAUNCH_NS plus LIFT_SPLIT_TILE_NS per round of 16 x 32 tiles over the CUs (level 3: 29 us a launch in one
//         round, level 2: 46 us in two); what follows the transform on the tail (subband MLPs, quantisation, the five stack
//         layers, rates) is LIFT_SPLIT_BASE_NS.
//   Beside the pair the tail's launches wait for compute units to fall free: the chain took 3.0-3.1 ms instead of 0.95,
//   LIFT_SPLIT_STRETCH_PERMILLE / 1000 times as long, and ended 30-200 us before the pair did.  The fork pays while the
//   stretched tail still ends before the main block does; past that the main stream would wait at the join for a chain that
//   runs three times slower than it would have alone.
constexpr int64_t LIFT_SPLIT_MAIN_PS = 537000;          // per pixel on ONE CU (x pixels / CUs = the block's time)
constexpr int64_t LIFT_SPLIT_LAUNCH_NS = 12000;
constexpr int64_t LIFT_SPLIT_TILE_NS = 17000;
constexpr int64_t LIFT_SPLIT_BASE_NS = 320000;
constexpr int64_t LIFT_SPLIT_STRETCH_PERMILLE = 3200;

// The tail alone, in ns: the lifting levels k .. levels - 1 and what follows them.
inline int64_t lift_split_tail_ns(int64_t Z, int64_t H, int64_t W, int levels, int cus, int k) {
    int64_t ns = LIFT_SPLIT_BASE_NS;
    for (int lev = k; lev < levels; ++lev) {
        const int64_t hh = (H >> lev) / 2, w = W >> lev, wh = w / 2;
        // 4 row steps on (hh, w), then 4 steps of the paired column passes on 2 x (hh, wh)
        const int64_t row = Z * ((hh + 15) / 16) * ((w + 31) / 32), col = 2 * Z * ((hh + 15) / 16) * ((wh + 31) / 32);
        ns += 4 * (LIFT_SPLIT_LAUNCH_NS + (row + cus - 1) / cus * LIFT_SPLIT_TILE_NS);
        ns += 4 * (LIFT_SPLIT_LAUNCH_NS + (col + cus - 1) / cus * LIFT_SPLIT_TILE_NS);
    }
    return ns;
}

// The main stream's independent block, in ns: pair and context MLP of the levels 0 .. k - 2.
inline int64_t lift_split_main_ns(int64_t Z, int64_t H, int64_t W, int cus, int k) {
    int64_t px = 0;
    for (int i = 0; i + 2 <= k; ++i) px += Z * (H >> (i + 1)) * (W >> (i + 1));
    return px * LIFT_SPLIT_MAIN_PS / cus / 1000;
}

// Z = planes x images, H x W the image, cus = compute units.  -> the level to fork at, or 0: fewer than 3 levels (nothing
// coarser than the level the main block needs), an unknown CU count, or a main block too short to hide the stretched tail.
inline int lift_split_level(int64_t Z, int64_t H, int64_t W, int levels, int cus) {
    if (levels < 3 || Z < 1 || H < 1 || W < 1 || cus < 1) return 0;
    const int k = LIFT_SPLIT_LEVEL;
    const int64_t tail = lift_split_tail_ns(Z, H, W, levels, cus, k), main_ns = lift_split_main_ns(Z, H, W, cus, k);
    return main_ns * 1000 >= tail * LIFT_SPLIT_STRETCH_PERMILLE ? k : 0;
}

}  // namespace lldwt
