"""Descriptor validation of the seven plan kinds (csrc/tvam_plan.h: TvamPlanKind) against what the library of
the commit before the kinds answered: tests/golden/plan_refusals.json, section "create", recorded by
tests/golden/make_plan_refusals.py.  Every base descriptor, each single fault and each pair of faults,
through every create entry, host segment dumper and tvam_row_slices: the same return code and the same
tvam_last_error() string, byte for byte.  No GPU is needed (validation returns before any device call); with
one, an accepted descriptor becomes a plan, which is destroyed: both count as accepted."""
import importlib.util
import os

import pytest

from drtvam_amd import _abi

_spec = importlib.util.spec_from_file_location(
    "make_plan_refusals", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_plan_refusals.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def ref():
    return rec.load()["create"]


def test_matrix_is_the_recorded_one(ref):
    cases = rec.create_cases()
    n = len(rec.FAULTS)
    assert len(cases) == len(rec.BASES) * (1 + n + n * (n - 1) // 2) and len(ref["create"]) == len(cases)
    assert set(ref["create"]) == {cid for cid, _, _ in cases} and ref["entries"] == list(rec.ENTRIES)
    assert set(ref["payload"]) == set(rec.payload_cases())
    for k in rec.BASES:  # each base is accepted by its kind's entry
        home = rec.ENTRIES.index(rec.HOME[k])
        assert ref["outcomes"][ref["create"][k][home]] == rec.ACCEPTED, k


@pytest.mark.parametrize("kind", rec.BASES)
def test_create_entries_answer_as_before(ref, kind):
    lib = _abi.load_library()
    n = 0
    for cid, k, faults in rec.create_cases():
        if k != kind:
            continue
        want = [ref["outcomes"][i] for i in ref["create"][cid]]
        for entry, w in zip(rec.ENTRIES, want):
            got = rec.run_entry(lib, entry, rec.faulty(k, faults))
            assert got == w, (cid, entry)
            n += 1
    assert n == len(rec.ENTRIES) * (1 + len(rec.FAULTS) * (len(rec.FAULTS) + 1) // 2)


def test_payload_refusals_answer_as_before(ref):
    lib = _abi.load_library()
    for cid, fn in rec.payload_cases().items():
        want = ref["outcomes"][ref["payload"][cid]]
        assert want != rec.ACCEPTED, cid
        assert fn(lib) == want, cid
