"""Recorder of tests/golden/plan_refusals.json: what the library of the commit before the plan kinds
(csrc/tvam_plan.h: TvamPlanKind) answered, as (return code, tvam_last_error()) pairs.

    TVAM_LIB=<libtvam.so built from that commit> python tests/golden/make_plan_refusals.py            # section "create"
    TVAM_LIB=<the same> python tests/golden/make_plan_refusals.py --gpu                               # section "calls" (needs a GPU)
    python tests/golden/make_plan_refusals.py --compare [--gpu]    # the current library against the file

"create" (no GPU needed: descriptor validation returns before any device call; tests/test_plan_kinds.py):
for each base descriptor (BASES: one or two per plan kind, film 8^3, 2 patterns, a 4 x 4 crop), every single
fault of FAULTS and every pair of them, through every entry of ENTRIES: the seven create calls (the reflect entry with
and without inserts), the three host segment dumpers with n_rays = 0 and tvam_row_slices.  Then PAYLOADS: the
refusals of what travels beside the descriptor, alone and after a descriptor fault.  An accepted descriptor
ends in hipSetDevice without a GPU and in a plan (destroyed at once) with one: both are recorded as [0, ""].

"calls" (tests/test_gpu_plan_kind_calls.py): one tiny plan of each kind (the scenes of tests/*_model.py, film
12^3, 3 angles, a 5 x 4 crop) through the eleven per-call entries that refuse plans by kind, with an empty
sparse active set where the entry takes one, so that an accepted call launches nothing; tvam_radon and
tvam_adjoint_slices take none and run on the tiny film.

The file holds a table of distinct outcomes and, per case, one index per entry."""
import ctypes
import itertools
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

from drtvam_amd import _abi  # noqa: E402

PATH = os.path.join(HERE, "plan_refusals.json")
ACCEPTED = [0, ""]


def _box(lo, hi):
    """12 triangles of an axis-aligned box, wound outwards: float32 [12, 3, 3]."""
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    v = np.array([[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0],
                  [x0, y0, z1], [x1, y0, z1], [x1, y1, z1], [x0, y1, z1]], np.float32)
    f = [(0, 2, 1), (0, 3, 2), (4, 5, 6), (4, 6, 7), (0, 1, 5), (0, 5, 4),
         (1, 2, 6), (1, 6, 5), (2, 3, 7), (2, 7, 6), (3, 0, 4), (3, 4, 7)]
    return np.ascontiguousarray(v[np.array(f)])


OUTER, INNER = _box((-0.8, -0.8, -1.0), (0.8, 0.8, 1.0)), _box((-0.7, -0.7, -0.9), (0.7, 0.7, 0.9))
INSERT = _box((-0.2, -0.15, -0.1), (0.2, 0.15, 0.1))
FAR_INSERT = INSERT + np.float32(5.0)  # outside the resin
FLAT = np.zeros((1, 3, 3), np.float32)  # a zero-area triangle
BLACK = _box((0.3, 0.3, -0.1), (0.4, 0.4, 0.1))[:1]
VIAL = _abi.TvamDoubleVial(0.8, 0.7, 0.4, 0.3, 1.5, 1.5, 1.4)
BAD_VIAL = _abi.TvamDoubleVial(0.7, 0.8, 0.4, 0.3, 1.5, 1.5, 1.4)


# ------------------------------------------------------------------------------------------ section "create"
def base_desc(kind):
    d = _abi.default_desc()
    d.film_res[:] = (8, 8, 8)
    d.n_patterns, d.res_x, d.res_y = 2, 16, 16
    d.crop_x, d.crop_y, d.crop_offset_x, d.crop_offset_y = 4, 4, 6, 6
    d.pixel_size_x = d.pixel_size_y = 0.1
    d.vial_r, d.vial_r_ext, d.vial_height, d.vial_ior, d.medium_ior = 0.7, 0.8, 2.0, 1.5, 1.4
    d.sigma_t, d.focus_distance, d.aperture_radius = 0.5, 20.0, 0.5
    lens = kind not in ("plain", "plain_cyl")
    d.projector_type = _abi.PROJECTOR_LENS if lens else _abi.PROJECTOR_COLLIMATED
    d.vial_type = {"plain_cyl": _abi.VIAL_CYLINDRICAL, "traced": _abi.VIAL_CYLINDRICAL, "mesh": _abi.VIAL_CUSTOM,
                   "double": _abi.VIAL_DOUBLE_CYLINDRICAL, "reflect": _abi.VIAL_CYLINDRICAL}.get(kind, _abi.VIAL_INDEX_MATCHED)
    if kind == "reflect":
        d.transmission_only = 0
    return d


BASES = ("plain", "plain_cyl", "cone", "traced", "mesh", "double", "inserts", "reflect")
# the create entry that accepts each base
HOME = {"plain": "create", "plain_cyl": "create", "cone": "create", "traced": "traced", "mesh": "mesh",
        "double": "double", "inserts": "inserts", "reflect": "reflect0"}


def _lens(d):
    if d.projector_type == _abi.PROJECTOR_COLLIMATED:
        d.projector_type = _abi.PROJECTOR_LENS


def _f_focus(d, k):
    _lens(d)
    d.focus_distance = 0.0


def _f_aperture(d, k):
    _lens(d)
    d.aperture_radius = -1.0


def _f_target(d, k):
    d.film_channels = 2
    d.set_target(INSERT)


def _f_ratio(d, k):
    d.sensor_type, d.majorant = _abi.SENSOR_RATIO, 2.0


def _f_rr(d, k):  # one below the kind's rule
    d.rr_depth = {"plain": 0, "cone": 0, "inserts": 0, "reflect": 0, "double": min(d.max_depth, 7) - 2}.get(k, 1)


def _f_geometry(d, k):
    if k == "mesh":
        d.vial_ior = 0.0
    elif k in ("double", "inserts", "reflect"):
        d.vial_height = 0.0
    elif k == "traced":
        d.vial_r_ext = d.vial_r
    elif k == "cone":
        d.vial_type = _abi.VIAL_SQUARE
    else:
        d.vial_r = 0.0


def _f_vial(d, k):  # wrong vial_type for the kind's entry
    d.vial_type = _abi.VIAL_INDEX_MATCHED if k in ("traced", "mesh", "double") else _abi.VIAL_CUSTOM


def _f_vial2(d, k):
    d.vial_type = _abi.VIAL_SQUARE if k in ("mesh", "double") else _abi.VIAL_DOUBLE_CYLINDRICAL


FAULTS = {
    "focus": _f_focus,
    "aperture": _f_aperture,
    "occluders": lambda d, k: d.set_occluders(BLACK),
    "albedo": lambda d, k: setattr(d, "albedo", 0.5),
    "ratio": _f_ratio,
    "delta": lambda d, k: setattr(d, "sensor_type", _abi.SENSOR_DELTA),
    "channels": _f_target,
    "slab": lambda d, k: setattr(d, "slab_end", 4),
    "transmission": lambda d, k: setattr(d, "transmission_only", 0 if d.transmission_only else 1),
    "rr": _f_rr,
    "geometry": _f_geometry,
    "vial": _f_vial,
    "vial2": _f_vial2,
    "vial99": lambda d, k: setattr(d, "vial_type", 99),
    "abi": lambda d, k: setattr(d, "abi_version", 99),
    "projector": lambda d, k: setattr(d, "projector_type", 7),
    "crop": lambda d, k: setattr(d, "crop_offset_x", 14),
    "bbox": lambda d, k: d.bbox_max.__setitem__(0, d.bbox_min[0]),
    "slab_range": lambda d, k: (setattr(d, "slab_begin", 5), setattr(d, "slab_end", 3)),
    "pixel": lambda d, k: setattr(d, "pixel_size_x", 0.0),
    "active_base": lambda d, k: setattr(d, "active_base", -1),
}


def create_cases():
    """[(case id, base kind, fault names)]: each base, its single faults and their pairs, in a fixed order."""
    out = []
    for k in BASES:
        out.append((k, k, ()))
        out += [(f"{k}+{a}", k, (a,)) for a in FAULTS]
        out += [(f"{k}+{a}+{b}", k, (a, b)) for a, b in itertools.combinations(FAULTS, 2)]
    return out


def faulty(kind, faults):
    d = base_desc(kind)
    for f in faults:
        FAULTS[f](d, kind)
    return d


def _outcome(lib, rc, plan=None):
    """(rc, message) as recorded; an accepted descriptor (a plan, or hipSetDevice's failure without a GPU) is
    ACCEPTED, and its plan is destroyed."""
    if plan is not None and plan.value:
        lib.tvam_plan_destroy(plan)
    msg = lib.tvam_last_error().decode(errors="replace") if rc else ""
    if rc == 0 or (rc == _abi.TVAM_ERR_HIP and msg.startswith("hipSetDevice")):
        return list(ACCEPTED)
    return [int(rc), msg]


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _inserts(tris):
    return _abi.insert_array([(t, 1.6, 1.4) for t in tris]), len(tris)


def _create(lib, entry, d, outer=OUTER, inner=INNER, vial=VIAL, ins=(INSERT,)):
    plan = ctypes.c_void_p()
    ref, out = ctypes.byref(d), ctypes.byref(plan)
    if entry == "create":
        rc = lib.tvam_plan_create(ref, 0, out)
    elif entry == "traced":
        rc = lib.tvam_plan_create_traced(ref, 0, out)
    elif entry == "mesh":
        rc = lib.tvam_plan_create_mesh(ref, _ptr(outer), 0 if outer is None else len(outer), _ptr(inner),
                                       0 if inner is None else len(inner), 0, out)
    elif entry == "double":
        rc = lib.tvam_plan_create_double(ref, None if vial is None else ctypes.byref(vial), 0, out)
    elif entry in ("inserts", "reflect", "reflect0"):
        arr, n = _inserts(() if entry == "reflect0" else ins)
        fn = lib.tvam_plan_create_inserts if entry == "inserts" else lib.tvam_plan_create_reflect
        rc = fn(ref, arr, n, 0, out)
    else:
        raise KeyError(entry)
    return _outcome(lib, rc, plan)


def _segments(lib, entry, d, ins=(INSERT,), n_rays=0, u=None):
    """The host segment dumpers; n_rays = 0 returns after the validation."""
    o = np.zeros((max(n_rays, 1), 3), np.float32)
    nseg = np.zeros(max(n_rays, 1), np.int32)
    if entry == "traced_segments":
        return _outcome(lib, lib.tvam_traced_segments(ctypes.byref(d), o.ctypes.data, o.ctypes.data, n_rays, None))
    arr, n = _inserts(() if entry == "reflect0_segments" else ins)
    fn = lib.tvam_insert_segments if entry == "insert_segments" else lib.tvam_reflect_segments
    return _outcome(lib, fn(ctypes.byref(d), arr, n, o.ctypes.data, o.ctypes.data, n_rays, _ptr(u), 0, None,
                            nseg.ctypes.data))


def _row_slices(lib, d):
    rows = np.zeros(64, np.int32)
    return _outcome(lib, lib.tvam_row_slices(ctypes.byref(d), rows.ctypes.data))


CREATES = ("create", "traced", "mesh", "double", "inserts", "reflect", "reflect0")
DUMPERS = ("traced_segments", "insert_segments", "reflect_segments", "reflect0_segments")
ENTRIES = CREATES + DUMPERS + ("row_slices",)


def run_entry(lib, entry, d):
    if entry in CREATES:
        return _create(lib, entry, d)
    if entry in DUMPERS:
        return _segments(lib, entry, d)
    return _row_slices(lib, d)


def payload_cases():
    """{case id: callable(lib) -> outcome}: what travels beside the descriptor, refused; each alone and
    after a descriptor fault (the descriptor's message comes first)."""
    out = {}
    for tag, faults in (("", ()), ("+albedo", ("albedo",))):
        m, dv, ins, rf = (lambda k=k, f=faults: faulty(k, f) for k in ("mesh", "double", "inserts", "reflect"))
        out |= {
            f"mesh{tag}/outer_null": lambda lib, m=m: _create(lib, "mesh", m(), outer=None),
            f"mesh{tag}/inner_empty": lambda lib, m=m: _create(lib, "mesh", m(), inner=INNER[:0]),
            f"mesh{tag}/outer_zero_area": lambda lib, m=m: _create(lib, "mesh", m(), outer=FLAT),
            f"mesh{tag}/inner_zero_area": lambda lib, m=m: _create(lib, "mesh", m(), inner=FLAT),
            f"double{tag}/null": lambda lib, dv=dv: _create(lib, "double", dv(), vial=None),
            f"double{tag}/radii": lambda lib, dv=dv: _create(lib, "double", dv(), vial=BAD_VIAL),
            f"inserts{tag}/none": lambda lib, ins=ins: _create(lib, "inserts", ins(), ins=()),
            f"inserts{tag}/outside": lambda lib, ins=ins: _create(lib, "inserts", ins(), ins=(INSERT, FAR_INSERT)),
            f"inserts{tag}/zero_area": lambda lib, ins=ins: _create(lib, "inserts", ins(), ins=(FLAT,)),
            f"inserts{tag}/segments_none": lambda lib, ins=ins: _segments(lib, "insert_segments", ins(), ins=()),
            f"inserts{tag}/segments_outside": lambda lib, ins=ins: _segments(lib, "insert_segments", ins(), ins=(FAR_INSERT,)),
            f"reflect{tag}/outside": lambda lib, rf=rf: _create(lib, "reflect", rf(), ins=(FAR_INSERT,)),
            f"reflect{tag}/segments_outside": lambda lib, rf=rf: _segments(lib, "reflect_segments", rf(), ins=(FAR_INSERT,)),
            f"reflect{tag}/segments_u_null": lambda lib, rf=rf: _segments(lib, "reflect_segments", rf(), n_rays=1),
            f"reflect{tag}/index_matched_none": lambda lib, f=faults: _create(lib, "reflect0", _im_reflect(f)),
            f"reflect{tag}/index_matched_none_segments": lambda lib, f=faults: _segments(lib, "reflect0_segments", _im_reflect(f)),
        }
    return out


def _im_reflect(faults):
    d = faulty("reflect", faults)
    d.vial_type = _abi.VIAL_INDEX_MATCHED
    return d


def record_create(lib):
    """{"outcomes": [[rc, message]], "entries": [...], "create": {case: [outcome index per entry]}, "payload": {case: index}}"""
    table, index = [], {}

    def ix(o):
        key = (o[0], o[1])
        if key not in index:
            index[key] = len(table)
            table.append(o)
        return index[key]

    create = {cid: [ix(run_entry(lib, e, faulty(k, faults))) for e in ENTRIES] for cid, k, faults in create_cases()}
    payload = {cid: ix(fn(lib)) for cid, fn in payload_cases().items()}
    return {"outcomes": table, "entries": list(ENTRIES), "create": create, "payload": payload}


# ------------------------------------------------------------------------------------------- section "calls"
CALLS = ("radon", "corner", "forward_slices", "adjoint_slices", "forward_dsigma", "adjoint_dsigma",
         "forward_dprojector", "adjoint_dprojector", "plan_rays", "plan_segments", "plan_insert_segments")
PLANS = ("plain", "plain_cyl", "cone", "traced", "mesh", "double", "inserts", "reflect", "reflect_inserts")


def _shrink(d, off_x, off_y):
    d.film_res[:] = (12, 12, 12)
    d.n_patterns = 3
    d.crop_x, d.crop_y, d.crop_offset_x, d.crop_offset_y = 5, 4, off_x, off_y
    return d


def plan_desc(name, meshdir):
    import double_vial_model as dv
    import insert_model as im
    import mesh_vial_model as mv
    import projector_model as pm
    import reflect_model as rm
    import traced_vial_model as tv
    if name == "plain":
        return _shrink(pm.projector_scene("collimated", regular=True), 9, 8)
    if name == "plain_cyl":
        d = _shrink(tv.traced_scene("cylindrical", "collimated", True), 41, 6)
        d.set_traced_vial(False)
        return d
    if name == "cone":
        return _shrink(pm.projector_scene("lens"), 9, 8)
    if name == "traced":
        return _shrink(tv.traced_scene("square", "lens", False), 21, 12)
    if name == "mesh":
        return _shrink(mv.custom_scene("lens", "cuvette"), 9, 8)
    if name == "double":
        return _shrink(dv.double_scene("lens", False), 32, 2)
    if name == "inserts":
        return _shrink(im.insert_scene(meshdir, "cylindrical", "lens", False, inserts=("prism", "u")), 9, 8)
    if name == "reflect":
        return _shrink(rm.reflect_scene(meshdir, "cylindrical", "collimated", True), 9, 8)
    if name == "reflect_inserts":
        return _shrink(rm.reflect_scene(meshdir, "index_matched", "lens", False, inserts=("u",)), 9, 8)
    raise KeyError(name)


def run_calls(lib, name, meshdir):
    """{call: outcome} of one tiny plan through CALLS."""
    import torch
    from drtvam_amd.engine import Projection
    dev = torch.device("cuda", 0)
    d = plan_desc(name, meshdir)
    proj = Projection(d, dev)
    p = proj._plan
    rz, ry, rx, _ = proj.film_shape
    n = proj.n_dense
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)
    data, pix = z(4), z(4, dt=torch.int32)  # an empty sparse set: valid pointers, n_active = 0
    film, grad, dense = z(rz, ry, rx), z(rz, ry, rx), z(n)
    g = z(1, dt=torch.float64)
    segs, nseg = z(4, 3, 8), z(4, dt=torch.int32)
    P = lambda t: t.data_ptr()
    calls = {
        "radon": lambda: lib.tvam_radon(p, None, 0, 1, 0, 3, P(dense), None),
        "corner": lambda: lib.tvam_corner(p, P(pix), 0, 1.0, 0.1, P(dense), None, None),
        "forward_slices": lambda: lib.tvam_forward_slices(p, P(data), P(pix), 0, 1, 0, 0, rz, P(film), None),
        "adjoint_slices": lambda: lib.tvam_adjoint_slices(p, P(grad), n, 0, rz, 0, d.crop_y, P(dense), None),
        "forward_dsigma": lambda: lib.tvam_forward_dsigma(p, P(data), P(pix), 0, 1, 0, P(film), None),
        "adjoint_dsigma": lambda: lib.tvam_adjoint_dsigma(p, P(data), P(grad), P(pix), 0, 1, 0, P(g), None),
        "forward_dprojector": lambda: lib.tvam_forward_dprojector(p, 0, P(data), P(pix), 0, 1, 0, P(film), None),
        "adjoint_dprojector": lambda: lib.tvam_adjoint_dprojector(p, 0, P(data), P(grad), P(pix), 0, 1, 0, P(g), None),
        "plan_rays": lambda: lib.tvam_plan_rays(p, P(pix), 0, 1, 0, P(segs), None),
        "plan_segments": lambda: lib.tvam_plan_segments(p, P(pix), 0, 1, 0, P(segs), None),
        "plan_insert_segments": lambda: lib.tvam_plan_insert_segments(p, P(pix), 0, 1, 0, 3, P(segs), P(nseg), None),
    }
    out = {}
    with torch.cuda.device(dev):
        for c in CALLS:
            rc = calls[c]()
            out[c] = [int(rc), lib.tvam_last_error().decode(errors="replace") if rc else ""]
        torch.cuda.synchronize(dev)
    out["path"] = [int(lib.tvam_plan_path(p)), ""]
    proj.close()
    return out


def record_calls(lib):
    with tempfile.TemporaryDirectory() as meshdir:
        return {name: run_calls(lib, name, meshdir) for name in PLANS}


# -------------------------------------------------------------------------------------------------- main
def load():
    with open(PATH) as f:
        return json.load(f)


def differences(got, ref):
    """Readable lines, one per differing case, of two sections in the file's layout."""
    lines = []
    if "outcomes" in got:
        g, r = got["outcomes"], ref["outcomes"]
        if got["entries"] != ref["entries"] or set(got["create"]) != set(ref["create"]) or set(got["payload"]) != set(ref["payload"]):
            lines.append("the case lists differ")
            return lines
        for cid, row in ref["create"].items():
            for e, a, b in zip(ref["entries"], got["create"][cid], row):
                if g[a] != r[b]:
                    lines.append(f"{cid} via {e}: {g[a]} != {r[b]}")
        for cid, b in ref["payload"].items():
            if g[got["payload"][cid]] != r[b]:
                lines.append(f"{cid}: {g[got['payload'][cid]]} != {r[b]}")
    else:
        for name in ref:
            for c, b in ref[name].items():
                if got[name][c] != b:
                    lines.append(f"{name} {c}: {got[name][c]} != {b}")
    return lines


def main(argv):
    lib = _abi.load_library()
    section = "calls" if "--gpu" in argv else "create"
    got = record_calls(lib) if section == "calls" else record_create(lib)
    if "--compare" in argv:
        diff = differences(got, load()[section])
        print("\n".join(diff[:50]))
        print(f"{section}: {len(diff)} differences")
        return 1 if diff else 0
    doc = load() if os.path.exists(PATH) else {}
    doc[section] = got
    with open(PATH, "w") as f:
        json.dump(doc, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    if section == "create":
        n = len(got["create"]) * len(ENTRIES) + len(got["payload"])
        acc = sum(got["outcomes"][i] == ACCEPTED for row in got["create"].values() for i in row)
        print(f"create: {n} cases, {len(got['outcomes'])} distinct outcomes, {acc} accepted; file {os.path.getsize(PATH)} B")
    else:
        for name, row in got.items():
            print(name, {c: o[0] for c, o in row.items()})
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
