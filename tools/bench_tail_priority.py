"""bench.py with the tail stream of the forked eval step at a given priority (ops.set_tail_priority: -1 high, 0 default):

    python tools/bench_tail_priority.py PRIORITY [bench.py arguments]

The priority comparison of DESIGN.md 9 item 7 (profiles/r15_overlap.json) alternates `bench.py`, this with -1 and this with 0."""
import os
import runpy
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

if __name__ == "__main__":
    from imagecompressionlearnedliftingandlearnedtreebasedmodels_amd import ops
    ops.set_tail_priority(int(sys.argv[1]))
    sys.argv = [os.path.join(REPO, "bench.py")] + sys.argv[2:]
    runpy.run_path(sys.argv[0], run_name="__main__")
