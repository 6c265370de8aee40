"""GPU: the bits of the fused lifting step (k_lift_fused_f16, eval path), pinned by tests/golden/lift_step_digests.json, which was
recorded at the commit before the kernel's issue work beside the MFMAs was cut (the view sets read
from the kernel-argument segment where they are used, unsigned run decoding).  Such changes remove or replace instructions that
produce nothing new, so no output bit may move -- and every diagnostics form of the kernel is compiled from the same source, so
none of them could be the reference.  Every case of
tests/golden/make_lift_digests.py is recomputed and its sha256 compared: five step shapes (one with a tile that is interior and
continues a run), both orientations, three precision modes, batch 2 and the smallest batch at which the dispatch takes the whole
column as one run, flags 0 and 32, one constant image, and one level through lifting_forward (the paired L / H column launch).
The one-run batch follows from the device's CU count, which therefore has to be the recorded one: a fixture recorded on another
device says nothing here, and the test fails instead of skipping."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_lift_digests", os.path.join(GOLDEN, "make_lift_digests.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)

with open(os.path.join(GOLDEN, "lift_step_digests.json")) as _f:
    _FIXTURE = json.load(_f)
WANT, NCU = _FIXTURE["cases"], int(_FIXTURE["provenance"]["cu_count"])
CASES = mk.cases(NCU)                                              # named from the recorded CU count: collected without a device


def test_the_device_and_the_fixture_match():
    assert mk.cu_count() == NCU
    names = [c[0] for c in CASES]
    assert sorted(names) == sorted(WANT) and len(set(names)) == len(names)
    # 48 x 96 at its one-run batch: the middle tile of the middle column is interior and continues a run
    b = mk.batch_for_whole_column_runs(48, 96, NCU)
    assert mk.dispatch_run_length(mk.P * b, 48, 96, NCU) == 3 and "step/48x96/v1/b%d/f0/f16x3" % b in WANT


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bits_are_those_of_the_fixture(case):
    assert mk.cu_count() == NCU
    outs, given = mk.run(case)
    for t, g in zip(outs, given):
        assert bool(torch.isfinite(t).all()), case[0]
        assert not torch.equal(t, g), case[0]                      # the step did run
    assert mk.digest(outs) == WANT[case[0]], case[0]
