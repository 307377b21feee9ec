"""Recorder of tests/golden/ray3d_parent_<walk>.npz: what the 3-D ray kernels of the commit before
csrc/tvam_ray3d.hip (tvam_cone.hip, tvam_double.hip, tvam_insert.hip) computed, one file per walk
instantiation.  tests/test_gpu_ray3d_parent.py renders the same cases (cases(), render()) and
compares.

    TVAM_LIB=<libtvam.so built from that commit> python tests/golden/make_ray3d_parent.py [outdir]
    python tests/golden/make_ray3d_parent.py --compare    # the current library against the files, bit by bit

Cases: film 12^3, 3 angles, a 5 x 4 crop of the DMD (60 rays per sample), the lens projector,
jittered, spp 2; the traced-glass walk once more collimated, regular, spp 1 ("col": the plain-store
adjoint epilogue and the collimated ray expressions).  The scenes and meshes are those of the GPU
suites (projector_model, mesh_vial_model, traced_vial_model, double_vial_model, insert_model)."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

SEED = 7
INSERT_SEGMENTS = 3
WALKS = ("one_nomesh", "one_glass", "one_mesh_lds", "one_mesh_global", "double", "insert_lds", "insert_global")


def path_of(walk, outdir=HERE):
    return os.path.join(outdir, f"ray3d_parent_{walk}.npz")


def _shrink(d, off_x, off_y):
    d.film_res[:] = (12, 12, 12)
    d.n_patterns = 3
    d.crop_x, d.crop_y, d.crop_offset_x, d.crop_offset_y = 5, 4, off_x, off_y
    return d


def cases(walk, meshdir):
    """{variant: (descriptor, spp)} of a walk: "jit" (lens, jittered, spp 2) and, for the glass, "col"."""
    import double_vial_model as dv
    import insert_model as im
    import mesh_vial_model as mv
    import projector_model as pm
    import traced_vial_model as tv
    if walk == "one_nomesh":
        return {"jit": (_shrink(pm.projector_scene("lens"), 9, 8), 2)}
    if walk == "one_glass":  # rows across the square vial's top edge (z = 2); columns across the tube's rim (6 .. 6.5)
        return {"jit": (_shrink(tv.traced_scene("square", "lens", False), 21, 12), 2),
                "col": (_shrink(tv.traced_scene("cylindrical", "collimated", True), 41, 6), 1)}
    if walk == "one_mesh_lds":
        return {"jit": (_shrink(mv.custom_scene("lens", "cuvette"), 9, 8), 2)}
    if walk == "one_mesh_global":  # 4096 triangles: the hierarchy read from global memory
        return {"jit": (_shrink(mv.custom_scene("lens", "tube"), 9, 8), 2)}
    if walk == "double":  # columns on either side of the inner vial's rim (x = 3): one and two segments
        return {"jit": (_shrink(dv.double_scene("lens", False), 32, 2), 2)}
    if walk == "insert_lds":  # the U-piece: up to three segments
        return {"jit": (_shrink(im.insert_scene(meshdir, "cylindrical", "lens", False, inserts=("prism", "u"), max_depth=12,
                                                rr_depth=12), 9, 8), 2)}
    if walk == "insert_global":  # 432 triangles, and the roulette acts
        return {"jit": (_shrink(im.insert_scene(meshdir, "square", "lens", False, inserts=("fine", "u"), max_depth=16,
                                                rr_depth=2, extinction=0.2), 9, 8), 2)}
    raise KeyError(walk)


def inputs(d):
    """The pattern and the film gradient of a case (fixed; stored with the results)."""
    rng = np.random.default_rng(2024)
    n = d.n_patterns * d.crop_y * d.crop_x
    return (rng.uniform(0.02, 0.1, n).astype(np.float32),
            rng.uniform(-1.0, 1.0, (d.film_res[2], d.film_res[1], d.film_res[0])).astype(np.float32))


def render(walk, d, spp, pat, G):
    """Everything a plan of the case computes through the 3-D ray kernels, as numpy arrays."""
    import torch
    from drtvam_amd import _abi
    from drtvam_amd.engine import Projection
    dev = "cuda:0"
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    out = {}
    proj = Projection(d, dev)
    out["rays"] = proj.rays(None, None, spp, SEED).cpu().numpy()
    if walk == "double":
        out["segs"] = proj.segments(None, None, spp, SEED).cpu().numpy()
        out["nseg"] = (out["segs"][:, :, 3] != 0.0).sum(1).astype(np.int32)
    elif walk.startswith("insert"):
        segs, nseg = proj.insert_segments(None, None, spp, SEED, INSERT_SEGMENTS)
        out["segs"], out["nseg"] = segs.cpu().numpy(), nseg.cpu().numpy()
    out["grad"] = proj.adjoint(t(G), pat.size, None, spp, SEED).cpu().numpy()
    out["visits"] = np.int64(proj.count_visits(spp, SEED))
    dose = proj.forward(t(pat), None, spp, SEED).cpu().numpy()[..., 0]
    proj.close()
    if walk.startswith("insert"):  # any number of segments: the per-ray atomics alone
        out["dose_atomic"] = dose
    else:
        out["dose_binned"] = dose
        da = d.copy()
        da.flags |= _abi.FLAG_SCATTER_ATOMIC
        proj = Projection(da, dev)
        out["dose_atomic"] = proj.forward(t(pat), None, spp, SEED).cpu().numpy()[..., 0]
        proj.close()
    return out


def render_walk(walk, meshdir):
    out = {}
    for var, (d, spp) in cases(walk, meshdir).items():
        pat, G = inputs(d)
        out[f"{var}/pat"], out[f"{var}/G"] = pat, G
        for k, v in render(walk, d, spp, pat, G).items():
            out[f"{var}/{k}"] = v
    return out


def main(argv):
    compare = "--compare" in argv
    args = [a for a in argv if not a.startswith("--")]
    outdir = args[0] if args else HERE
    all_same = True
    with tempfile.TemporaryDirectory() as meshdir:
        for walk in WALKS:
            got = render_walk(walk, meshdir)
            if not compare:
                np.savez_compressed(path_of(walk, outdir), **got)
                size = os.path.getsize(path_of(walk, outdir))
            for var in sorted({k.split("/")[0] for k in got}):
                r = got[f"{var}/rays"]
                ns = got.get(f"{var}/nseg")
                print(f"{walk}/{var}: rays {len(r)} hit {int((r[:, 6] != 0).sum())} visits {int(got[f'{var}/visits'])} "
                      f"segments per ray {np.bincount(ns).tolist() if ns is not None else '-'} "
                      f"|grad| {np.abs(got[f'{var}/grad']).max():.4e} dose sum {got[f'{var}/dose_atomic'].sum():.6e}"
                      + ("" if compare else f" file {size} B"))
            if compare:
                ref = np.load(path_of(walk, outdir))
                for k in sorted(got):
                    a, b = np.asarray(got[k]), ref[k]
                    same = a.shape == b.shape and a.tobytes() == b.tobytes()
                    worst = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) if a.shape == b.shape else np.inf
                    scale = float(np.abs(b.astype(np.float64)).max())
                    all_same &= same or "dose" in k
                    print(f"  {walk}/{k}: {'bit-identical' if same else 'DIFFERS'} (largest |difference| {worst:.3e}, "
                          f"largest magnitude {scale:.3e})")
    if compare:
        print("everything except the forward doses bit-identical:", all_same)


if __name__ == "__main__":
    main(sys.argv[1:])
