"""Float64 NumPy model of the projector rays (test helper, no GPU): the TEA-scrambled PCG32
'independent' sampler, Mitsuba's concentric disk warp, get_ray of the collimated / telecentric /
lens projectors (projector.py:184-188, :220-234, :273-286), CircularMotion's to_world
(motion.py:26-36) and the medium segment behind the index-matched vial (open tube, front-facing
entry, spawn offset, exit through the wall; volume.py:191-216, :268).

Everything after the sampler's fp32 uniforms and the fp32 rotation angle is float64, so the model
is the exact-arithmetic answer the fp32 kernels are compared with."""
import numpy as np

ZC = 0.005                      # camera-space z of the near plane (sample_to_camera)
RAY_EPS = 1500.0 * 2.0 ** -24   # math::RayEpsilon<float>
TWO_PI_F = np.float32(6.2831855)


# --------------------------------------------------------------------------- sampler
def _tea(v0, v1, rounds=4):
    v0 = v0.astype(np.uint32).copy()
    v1 = v1.astype(np.uint32).copy()
    s = np.uint32(0)
    with np.errstate(over="ignore"):
        for _ in range(rounds):
            s = np.uint32((int(s) + 0x9E3779B9) & 0xFFFFFFFF)
            v0 += ((v1 << np.uint32(4)) + np.uint32(0xA341316C)) ^ (v1 + s) ^ ((v1 >> np.uint32(5)) + np.uint32(0xC8013EA4))
            v1 += ((v0 << np.uint32(4)) + np.uint32(0xAD90777D)) ^ (v0 + s) ^ ((v0 >> np.uint32(5)) + np.uint32(0x7E95761E))
    return v0, v1


class Sampler:
    """Vectorised PCG32 streams seeded like the 'independent' sampler: seed(seed, wavefront) draws
    stream i with (initstate, initseq) = tea(seed, i)."""
    MULT = np.uint64(0x5851F42D4C957F2D)

    def __init__(self, seed, streams):
        streams = np.asarray(streams, dtype=np.uint64)
        v0, v1 = _tea(np.full(streams.shape, seed & 0xFFFFFFFF, dtype=np.uint32),
                      (streams & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        self.state = np.zeros(streams.shape, dtype=np.uint64)
        self.inc = (v1.astype(np.uint64) << np.uint64(1)) | np.uint64(1)
        self.next_u32()
        with np.errstate(over="ignore"):
            self.state = self.state + v0.astype(np.uint64)
        self.next_u32()

    def next_u32(self):
        old = self.state
        with np.errstate(over="ignore"):
            self.state = old * self.MULT + self.inc
        xs = (((old >> np.uint64(18)) ^ old) >> np.uint64(27)).astype(np.uint32)
        rot = (old >> np.uint64(59)).astype(np.uint32)
        return (xs >> rot) | (xs << ((np.uint32(32) - rot) & np.uint32(31)))

    def next_float(self):
        """The fp32 uniform in [0, 1), as float64 (exact)."""
        bits = (self.next_u32() >> np.uint32(9)) | np.uint32(0x3F800000)
        return (bits.view(np.float32) - np.float32(1.0)).astype(np.float64)


# --------------------------------------------------------------------------- warp
def square_to_uniform_disk_concentric(u1, u2):
    u1, u2 = np.asarray(u1, np.float64), np.asarray(u2, np.float64)
    x, y = 2.0 * u1 - 1.0, 2.0 * u2 - 1.0
    q = np.abs(x) < np.abs(y)
    r = np.where(q, y, x)
    rp = np.where(q, x, y)
    zero = (x == 0.0) & (y == 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        phi = 0.25 * np.pi * rp / np.where(zero, 1.0, r)
    phi = np.where(q, 0.5 * np.pi - phi, phi)
    phi = np.where(zero, 0.0, phi)
    return r * np.cos(phi), r * np.sin(phi)


# --------------------------------------------------------------------------- rays
def camera_xy(desc, col, row, jx, jy):
    """tvam_ray_camera: ((0.5 - u) W a_x, (0.5 - v) H a_y), u = (col + jx) / W."""
    W, H = desc.res_x, desc.res_y
    ax, ay = float(np.float32(desc.pixel_size_x)), float(np.float32(desc.pixel_size_y))
    u = (col + jx) / W
    v = (row + jy) / H
    return (0.5 - u) * W * ax, (0.5 - v) * H * ay


def get_ray(desc, xc, yc, u1, u2):
    """Camera-space origin and unit direction of the plan's projector."""
    a = float(np.float32(desc.aperture_radius))
    F = float(np.float32(desc.focus_distance))
    dx, dy = square_to_uniform_disk_concentric(u1, u2)
    ax, ay = a * dx, a * dy
    z = np.zeros_like(xc)
    if desc.projector_type == 0:    # collimated: the pixel's point of the near plane, along +z
        o = np.stack([xc, yc, z + ZC], -1)
        d = np.stack([z, z, z + 1.0], -1)
        return o, d
    if desc.projector_type == 1:    # telecentric
        o = np.stack([xc + ax, yc + ay, z], -1)
        d = np.stack([-ax, -ay, z + (ZC + F)], -1)
    else:                           # lens
        o = np.stack([ax, ay, z], -1)
        d = np.stack([xc - ax, yc - ay, z + F], -1)
    return o, d / np.linalg.norm(d, axis=-1, keepdims=True)


def to_world(desc, alpha, o, d):
    """CircularMotion: camera (X, Y, Z) -> (c (D - Z) + s X, s (D - Z) - c X, Y)."""
    D = float(np.float32(desc.distance))
    c, s = np.cos(alpha), np.sin(alpha)
    ow = np.stack([c * (D - o[..., 2]) + s * o[..., 0], s * (D - o[..., 2]) - c * o[..., 0], o[..., 1]], -1)
    dw = np.stack([-c * d[..., 2] + s * d[..., 0], -s * d[..., 2] - c * d[..., 0], d[..., 1]], -1)
    return ow, dw


def to_camera(desc, alpha, p):
    """Inverse of to_world for points."""
    D = float(np.float32(desc.distance))
    c, s = np.cos(alpha), np.sin(alpha)
    return np.stack([s * p[..., 0] - c * p[..., 1], p[..., 2], D - (c * p[..., 0] + s * p[..., 1])], -1)


def angle_alpha(desc, angle, ut=None):
    """The rotation angle the fp32 code forms (motion.py:28), as float64."""
    t = np.asarray(angle, dtype=np.float32)
    if ut is not None:
        t = t + np.asarray(ut, dtype=np.float32)
    t = t / np.float32(desc.n_patterns)
    a = TWO_PI_F * t
    return (-a if desc.clockwise else a).astype(np.float64)


def _tube_hit(o, d, r, half):
    """Nearest t >= 0 of the open tube (inf where none) for rays [n, 3]."""
    A = d[:, 0] ** 2 + d[:, 1] ** 2
    B = 2.0 * (d[:, 0] * o[:, 0] + d[:, 1] * o[:, 1])
    C = o[:, 0] ** 2 + o[:, 1] ** 2 - r * r
    disc = B * B - 4.0 * A * C
    ok = disc >= 0.0
    sq = np.sqrt(np.where(ok, disc, 0.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        t0 = (-B - sq) / (2.0 * A)
        t1 = (-B + sq) / (2.0 * A)
    zn, zf = o[:, 2] + d[:, 2] * t0, o[:, 2] + d[:, 2] * t1
    near = ok & (t1 >= 0.0) & (t0 >= 0.0) & (np.abs(zn) <= half)
    far = ok & (t1 >= 0.0) & ~near & (np.abs(zf) <= half)
    t = np.where(near, t0, np.where(far, t1, np.inf))
    # distance of the decisions from their thresholds (for the tests' margin check)
    margin = np.minimum(np.abs(np.abs(zn) - half), np.abs(np.abs(zf) - half))
    return t, margin


def segment(desc, o, d):
    """Medium segment of world rays [n, 3]: hit, o2, maxt and the margin of the hit decision."""
    r, half = float(np.float32(desc.vial_r)), 0.5 * float(np.float32(desc.vial_height))
    n = o.shape[0]
    t0, m0 = _tube_hit(o, d, r, half)
    hit = np.isfinite(t0)
    t0s = np.where(hit, t0, 0.0)
    p = o + d * t0s[:, None]
    rp = np.hypot(p[:, 0], p[:, 1])
    nrm = np.stack([p[:, 0] / rp, p[:, 1] / rp, np.zeros(n)], -1)
    ndd = np.sum(nrm * d, -1)
    hit &= ndd < 0.0
    mag = (1.0 + np.max(np.abs(p), -1)) * RAY_EPS
    o2 = p - mag[:, None] * nrm
    t1, m1 = _tube_hit(o2, d, r, half)
    margin = np.where(hit, np.minimum(m0, m1), m0)
    hit &= np.isfinite(t1)
    return hit, o2, np.where(hit, t1, 0.0), margin


def model_rays(desc, pixels, streams, spp, seed):
    """The rays of active entries `pixels` (flat indices into the full DMD) whose sampler streams
    are streams[i] * spp + k: dict of o, d, hit, o2, maxt, margin, alpha (row i * spp + k)."""
    pixels = np.repeat(np.asarray(pixels, dtype=np.int64), spp)
    st = np.repeat(np.asarray(streams, dtype=np.uint64), spp) * np.uint64(spp) + \
        np.tile(np.arange(spp, dtype=np.uint64), len(streams))
    hw = desc.res_x * desc.res_y
    angle, pix = pixels // hw, pixels % hw
    row, col = pix // desc.res_x, pix % desc.res_x
    smp = Sampler(seed, st)
    jx = jy = np.full(pixels.shape, 0.5)
    if not desc.regular_sampling:
        jx, jy = smp.next_float(), smp.next_float()
    ut = smp.next_float() if desc.sample_time else None
    u1, u2 = smp.next_float(), smp.next_float()
    alpha = angle_alpha(desc, angle, ut)
    xc, yc = camera_xy(desc, col, row, jx, jy)
    oc, dc = get_ray(desc, xc, yc, u1, u2)
    o, d = to_world(desc, alpha, oc, dc)
    hit, o2, maxt, margin = segment(desc, o, d)
    return dict(o=o, d=d, hit=hit, o2=o2, maxt=maxt, margin=margin, alpha=alpha, xc=xc, yc=yc)


def dense_pixels(desc, a0=0, a1=None):
    """Flat full-DMD indices of the dense crop order of angles [a0, a1) (projector.py:90-98)."""
    a1 = desc.n_patterns if a1 is None else a1
    a, r, c = np.meshgrid(np.arange(a0, a1), np.arange(desc.crop_y), np.arange(desc.crop_x), indexing="ij")
    return (a * desc.res_y * desc.res_x + (desc.crop_offset_y + r) * desc.res_x + desc.crop_offset_x + c).ravel()


def ray_weight(desc, n_total, spp):
    """or_ray_weight in fp32 (projector.py:164-165, :187; common.py:111), times sigma_a / sigma_t."""
    area = np.float32(desc.pixel_size_x) * np.float32(desc.pixel_size_y) * np.float32(n_total)
    w = area / np.float32(n_total * spp)
    w = w * np.float32(desc.print_time)
    ss = np.float32(desc.albedo) * np.float32(desc.sigma_t)
    sa_st = np.float32((float(np.float32(desc.sigma_t)) - float(ss)) / float(np.float32(desc.sigma_t)))
    return np.float32(w * sa_st)


def inv_vol(desc):
    h = [(np.float32(desc.bbox_max[a]) - np.float32(desc.bbox_min[a])) / np.float32(desc.film_res[a]) for a in range(3)]
    return np.float32(1.0) / (h[0] * h[1] * h[2])


def projector_scene(kind="telecentric", height=40.0, regular=False, sample_time=False, aperture=2.0, lens_fov=False):
    """The shared small scene of the projector tests: film 40 x 36 x 20 voxels of 0.1 mm (more than
    one 32 x 32 x 16 brick on every axis, a multiple on none), DMD 24 x 20 px of 0.15 mm, 6 patterns,
    sigma_t 1 / mm (0.1 per voxel), aperture_radius / focus_distance = 0.1, distance = focus_distance."""
    from drtvam_amd.configs import desc_from_config
    F = 20.0
    proj = {"type": kind, "n_patterns": 6, "resx": 24, "resy": 20, "motion": "circular", "distance": F}
    if kind == "collimated":
        proj["pixel_size"] = 0.15
    else:
        proj |= {"aperture_radius": aperture, "focus_distance": F}
        if kind == "lens" and lens_fov:  # the same 0.15 mm pixel at the focus plane
            proj["fov"] = float(np.rad2deg(2 * np.arctan(0.15 * 24 / 2 / F)))
        else:
            proj["pixel_size"] = 0.15
    cfg = {
        "vial": {"type": "index_matched", "r": 2.9, "height": height,
                 "medium": {"ior": 1.0, "extinction": 1.0, "albedo": 0.0}},
        "projector": proj,
        "sensor": {"type": "dda", "scalex": 4.0, "scaley": 3.6, "scalez": 2.0,
                   "film": {"type": "vfilm", "resx": 36, "resy": 40, "resz": 20}},
        "target": {"analytic": "box_hole"},
        "loss": {"type": "threshold", "tl": 0.9, "tu": 0.95},
        "regular_sampling": regular,
    }
    d = desc_from_config(cfg)
    d.sample_time = int(sample_time)
    assert tuple(d.film_res) == (40, 36, 20), tuple(d.film_res)
    return d
