"""Host: the rule that says where, if anywhere, the eval step forks the lifting transform (lift_split_level, csrc/lift_split.h:
plain C++, compiled here into a small program; no GPU) at the shapes of BASELINE configs[1] .. [4] on 256 CUs: 0 below 3 levels,
otherwise monotone in the image size -- once the main stream's block hides the tail it keeps hiding it as the image grows --
and its two estimates against the figures they were fitted to."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "imagecompressionlearnedliftingandlearnedtreebasedmodels_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "lift_split.h"
int main(int argc, char** argv) {
    for (int i = 1; i + 4 < argc; i += 5) {
        const long long Z = std::atoll(argv[i]), H = std::atoll(argv[i + 1]), W = std::atoll(argv[i + 2]);
        const int L = std::atoi(argv[i + 3]), cus = std::atoi(argv[i + 4]);
        std::printf("%d %lld %lld\n", lldwt::lift_split_level(Z, H, W, L, cus),
                    (long long)lldwt::lift_split_tail_ns(Z, H, W, L, cus > 0 ? cus : 1, lldwt::LIFT_SPLIT_LEVEL),
                    (long long)lldwt::lift_split_main_ns(Z, H, W, cus > 0 ? cus : 1, lldwt::LIFT_SPLIT_LEVEL));
    }
    return 0;
}
"""

# (Z = planes x images, H, W, levels) of configs[1] .. [4]; configs[4] is 8 strips of 2160 x 480
CONFIGS = {1: (48, 256, 256, 3), 2: (24, 512, 512, 4), 3: (12, 1024, 1024, 4), 4: (24, 2160, 480, 4)}


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    d = tmp_path_factory.mktemp("lift_split")
    (d / "rule.cpp").write_text(PROGRAM)
    cxx = shutil.which("c++") or shutil.which("g++") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(d / "rule"), str(d / "rule.cpp")], check=True)

    def ask(cases):
        args = [str(v) for c in cases for v in c]
        out = subprocess.run([str(d / "rule")] + args, check=True, capture_output=True, text=True).stdout.splitlines()
        return [tuple(int(v) for v in line.split()) for line in out]
    return ask


def test_bench_shapes(rule):
    got = rule([CONFIGS[i] + (256,) for i in (1, 2, 3, 4)])
    # configs[1]: 48 x 128 x 128 level-0 pixels (1.65 ms) do not hide one stretched level and the stacks (0.55 ms x 3.2)
    assert [g[0] for g in got] == [0, 2, 2, 2]
    # the flagship, as traced: 0.95 ms of tail (16 lifting launches, the stacks, the small kernels) against 3.3 ms of level-0
    # pair and context MLP
    _, tail, main = got[1]
    assert 850_000 <= tail <= 1_050_000 and 3_200_000 <= main <= 3_400_000


def test_fewer_than_three_levels_and_edges(rule):
    got = rule([(24, 512, 512, 2, 256), (24, 512, 512, 1, 256), (48, 4096, 4096, 2, 256), (24, 512, 512, 4, 0), (0, 512, 512, 4, 256)])
    assert [g[0] for g in got] == [0, 0, 0, 0, 0]


@pytest.mark.parametrize("cfg", [1, 2, 3, 4])
def test_monotone_in_image_size(rule, cfg):
    """Both sides scaled by 2^j from 1/16 of the config's size to 4 times it, and each side alone: the answer never goes back to
    0 once it is 2, it is 0 at the small end, and 0 and 2 are the only answers."""
    Z, H, W, L = CONFIGS[cfg]
    unit = 1 << L
    both = [(Z, max(unit, (H >> 4 << j) // unit * unit), max(unit, (W >> 4 << j) // unit * unit), L, 256) for j in range(7)]
    tall = [(Z, max(unit, (H >> 4 << j) // unit * unit), W, L, 256) for j in range(7)]
    wide = [(Z, H, max(unit, (W >> 4 << j) // unit * unit), L, 256) for j in range(7)]
    for cases in (both, tall, wide):
        ans = [g[0] for g in rule(cases)]
        assert set(ans) <= {0, 2}
        assert ans == sorted(ans), (cases, ans)
    assert [g[0] for g in rule(both)][0] == 0
    # more images of the same size: the main block grows with them, the tail's launches only fill up
    ans = [g[0] for g in rule([(z, H >> 2, W >> 2, L, 256) for z in (1, 3, 6, 12, 24, 48, 96, 192)])]
    assert ans == sorted(ans)
