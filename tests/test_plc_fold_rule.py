"""Host: the rule that decides per launch whether k_plc_wino folds the channel blocks of a pixel tile into one workgroup
(plc_fold_pays, csrc/plc_fold.h: plain C++, compiled here into a small program; no GPU).  The three tree-pair launches of the
bench step (BASELINE configs[2]: 3 planes x 8 images at 256, 128 and 64 pixels, 243 channels = 2 blocks, 256 CUs) and the
crossover between them."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "imagecompressionlearnedliftingandlearnedtreebasedmodels_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "plc_fold.h"
int main(int argc, char** argv) {
    for (int i = 1; i + 2 < argc; i += 3)
        std::printf("%d\n", lldwt::plc_fold_pays(std::atoll(argv[i]), std::atoi(argv[i + 1]), std::atoi(argv[i + 2])) ? 1 : 0);
    std::printf("permille %d\n", lldwt::PLC_FOLD_SAVING_PERMILLE);
    return 0;
}
"""


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    d = tmp_path_factory.mktemp("plc_fold")
    (d / "rule.cpp").write_text(PROGRAM)
    cxx = shutil.which("c++") or shutil.which("g++") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(d / "rule"), str(d / "rule.cpp")], check=True)

    def ask(cases):
        args = [str(v) for c in cases for v in c]
        out = subprocess.run([str(d / "rule")] + args, check=True, capture_output=True, text=True).stdout.split()
        return [bool(int(v)) for v in out[:len(cases)]], int(out[-1])
    return ask


def _tiles(size):
    return (size // 32) * (size // 8)


def test_bench_launches(rule):
    """Level 0: 6 144 tiles x images, 24 folded rounds against 48; level 1: 1 536, 6 against 12; level 2: 384, 2 double-length rounds
    against 3 single ones: not folded."""
    n = [_tiles(s) * 24 for s in (256, 128, 64)]
    assert n == [6144, 1536, 384]
    got, permille = rule([(n[0], 256, 2), (n[1], 256, 2), (n[2], 256, 2)])
    assert got == [True, True, False]
    assert 0 < permille < 500            # a later pass saves a part of a workgroup's time, less than half of it


def test_crossover_and_edges(rule):
    got, permille = rule([
        (256, 256, 2),       # one folded round against two: pays whatever a pass saves
        (257, 256, 2),       # two folded rounds (4T - 2s) against three (3T): does not pay
        (512, 256, 2),       # 2 against 4: pays
        (513, 256, 2),       # 3 against 5: 6T - 3s > 5T unless s > T / 3
        (640, 256, 2),       # 3 against 5
        (641, 256, 2),       # 3 against 6: pays
        (6144, 256, 1),      # one channel block: nothing to fold
        (6144, 0, 2),        # CU count unknown: never fold
        (384, 256, 3),       # three blocks: 2 rounds of 3T - 2s against 5 of T
        (100000, 256, 2),    # many rounds: the partly filled last round does not matter
    ])
    assert permille < 333
    assert got == [True, False, True, False, False, True, False, False, False, True]
    # the rule as the launch states it, for every tile count around the bench's small launches
    cases = [(n, 256, 2) for n in range(1, 1500, 7)]
    got, _ = rule(cases)
    for (n, cus, nocb), g in zip(cases, got):
        folded, unfolded = -(-n // cus), -(-n * nocb // cus)
        assert g == (folded * (nocb * 1000 - (nocb - 1) * permille) < unfolded * 1000), n
