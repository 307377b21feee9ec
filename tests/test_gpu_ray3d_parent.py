"""The 3-D ray kernels (csrc/tvam_ray3d.hip: one march, record and export kernel over the walk
policies of tvam_ray3d.h) against what the three kernel families they replaced computed
(tvam_cone.hip, tvam_double.hip, tvam_insert.hip of the commit before): fixtures recorded on the
GPU from a build of that commit by tests/golden/make_ray3d_parent.py, one per walk instantiation.

Per case (film 12^3, 3 angles, a 5 x 4 DMD crop = 60 rays per sample; lens projector, jittered,
spp 2; the traced glass once more collimated, regular, spp 1): the exported rays, the segments and
their counts where the plan has them, the adjoint of a fixed film gradient, the visit count, and the
forward through the brick bins and through the per-ray atomics.  Integers are equal; float arrays
agree within RTOL of the array's largest magnitude, every ray compared.  (On the recording toolchain
everything but the forward doses is bit-identical, profiles/ray3d/equivalence.txt; the tolerance
keeps a later toolchain's cosf from breaking the test.)"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-4  # the project's parity bar

_spec = importlib.util.spec_from_file_location(
    "make_ray3d_parent", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_ray3d_parent.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

CASES = [(w, "jit") for w in rec.WALKS] + [("one_glass", "col")]


@pytest.fixture(scope="module")
def meshdir(tmp_path_factory):
    return tmp_path_factory.mktemp("ray3d_meshes")


@pytest.mark.parametrize("walk,var", CASES, ids=[f"{w}-{v}" for w, v in CASES])
def test_matches_parent(meshdir, walk, var):
    ref = np.load(rec.path_of(walk))
    d, spp = rec.cases(walk, meshdir)[var]
    pat, G = ref[f"{var}/pat"], ref[f"{var}/G"]
    got = rec.render(walk, d, spp, pat, G)
    want = {k.split("/", 1)[1]: ref[k] for k in ref.files if k.startswith(var + "/") and k not in (f"{var}/pat", f"{var}/G")}
    assert set(got) == set(want)
    n = 60 * spp
    assert got["rays"].shape == (n, 16) and want["rays"].shape == (n, 16)
    # integers: hit flags, segment counts, visits
    assert np.array_equal(got["rays"][:, 6], want["rays"][:, 6])
    assert int(got["visits"]) == int(want["visits"]) and int(want["visits"]) > 0
    if "nseg" in want:
        assert np.array_equal(got["nseg"], want["nseg"])
        if walk.startswith("insert"):
            assert want["segs"].shape == (n, rec.INSERT_SEGMENTS, 8) and want["nseg"].max() >= 3
        else:
            assert want["segs"].shape == (n, 2, 8) and (want["nseg"] == 1).any() and (want["nseg"] == 2).any()
    for k in sorted(want):
        if k in ("visits", "nseg"):
            continue
        a, b = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        scale = float(np.abs(b).max())
        err = float(np.abs(a - b).max())
        print(f"{walk}/{var} {k}: largest |difference| {err:.3e}, largest magnitude {scale:.3e}, "
              f"bit-identical {np.asarray(got[k]).tobytes() == want[k].tobytes()}")
        assert a.shape == b.shape and scale > 0.0
        assert err <= RTOL * scale, k
