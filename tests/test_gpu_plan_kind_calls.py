"""What the per-call entry points refuse of each plan kind (csrc/tvam_calls.hip: one switch on TvamPlanKind
per entry) against what the library of the commit before the kinds answered: tests/golden/plan_refusals.json,
section "calls", recorded on the GPU by tests/golden/make_plan_refusals.py --gpu.

One tiny plan per kind (film 12^3, 3 angles, a 5 x 4 crop; a collimated index-matched and a collimated
cylindrical plan, a reflect plan with and without inserts) through tvam_radon, tvam_corner, the slice entries,
the extinction and projector derivatives and the three ray exports, with an empty sparse active set where the
entry takes one: an accepted call returns 0 and launches nothing (tvam_radon and tvam_adjoint_slices run on
the tiny film).  The same return code and the same message, byte for byte; tvam_plan_path too."""
import importlib.util
import os

import pytest

from drtvam_amd import _abi

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "make_plan_refusals", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_plan_refusals.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def meshdir(tmp_path_factory):
    return tmp_path_factory.mktemp("plan_kind_meshes")


def test_every_kind_and_call_is_recorded():
    ref = rec.load()["calls"]
    assert set(ref) == set(rec.PLANS)
    for name in rec.PLANS:
        assert set(ref[name]) == set(rec.CALLS) | {"path"}
        for call in rec.CALLS:
            rc, msg = ref[name][call]
            assert (rc == 0) == (msg == ""), (name, call)
    # the 3-D ray kinds report bit 2 of tvam_plan_path, the collimated plans do not
    assert all((ref[n]["path"][0] & 4) == (0 if n.startswith("plain") else 4) for n in rec.PLANS)
    # every entry refuses some kind and serves another
    for call in rec.CALLS:
        codes = {ref[n][call][0] for n in rec.PLANS}
        assert 0 in codes and _abi.TVAM_ERR_UNSUPPORTED in codes, call


@pytest.mark.parametrize("name", rec.PLANS)
def test_calls_answer_as_before(meshdir, name):
    want = rec.load()["calls"][name]
    got = rec.run_calls(_abi.load_library(), name, meshdir)
    for call in rec.CALLS + ("path",):
        print(name, call, got[call])
        assert got[call] == want[call], (name, call)
