"""GPU: the bytes that the three coded entropy layers write from the filled weights, pinned by tests/golden/streams_n1.json.
Every case of tests/golden/make_streams.py is recomputed and compared -- the sha256 over the streams (the list of byte counts
for the estimating sink) and the sha256 over the dequantised tensors -- and, for the cases that write streams, the decoder
rebuilds exactly the encoder's tensors, in full and from first_level = 1.  The fixture's provenance entry is for the reader."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_streams", os.path.join(GOLDEN, "make_streams.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)

with open(os.path.join(GOLDEN, "streams_n1.json")) as _f:
    WANT = json.load(_f)["cases"]
CASES = mk.cases()


def test_the_fixture_holds_exactly_the_cases():
    names = [c[0] for c in CASES]
    assert sorted(names) == sorted(WANT) and len(set(names)) == len(names) == 39


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_streams_and_values_are_those_of_the_fixture(case):
    streams, tensors, decode = mk.run(case)
    assert mk.record(streams, tensors) == WANT[case[0]]
    if case[3] == "estimate":
        return
    full = decode(0)
    assert len(full) == len(tensors) and all(torch.equal(a, b) for a, b in zip(full, tensors))
    if case[1] == "generic":                                   # one level: nothing to reduce
        return
    tail = decode(1)
    want = [tensors[0]] + tensors[2:]
    assert len(tail) == len(want) and all(torch.equal(a, b) for a, b in zip(tail, want))
