"""Float64 models and checkers of the extinction derivative d dose / d sigma_t,
shared by test_dsigma_model.py (CPU) and the GPU tests.

The weight.  A visit that starts at in-medium path length T0 and lasts dt deposits
e^{-s T0} - e^{-s (T0 + dt)}; its derivative in s = sigma_t is
    w'(T0, dt) = (T0 + dt) e^{-s (T0 + dt)} - T0 e^{-s T0}                  (first form: w_exact)
               = e^{-s T0} (dt (1 - q) - T0 q),  q = 1 - e^{-s dt}          (second form: the fp32 code)

Ground truth of the tangent film T = d dose / d sigma_t: the central difference of a float64 dose at
sigma +- h (fd_tangent), accepted only when it has converged (assert_converged)."""
import numpy as np

U = 2.0 ** -24  # unit roundoff of fp32: one rounded operation has relative error <= U
RTOL = 1e-4     # the project's forward bars: relative L2, and per voxel against max |reference|


def w_exact(s, T0, dt):
    """w' in float64 from its first form, at the fp32 values of the arguments."""
    s = np.float64(np.float32(s))
    T0 = np.asarray(np.float32(T0), np.float64)
    dt = np.asarray(np.float32(dt), np.float64)
    return (T0 + dt) * np.exp(-s * (T0 + dt)) - T0 * np.exp(-s * T0)


# weight_bound: |fp32 w' - w'| <= (K + 3 s (T0 + dt)) U e^{-s T0} (|A| + |B|), A = dt (1 - q), B = T0 q,
# for the expression as tvam_dsig_weight writes it,  w = E0 * (dt * omq - T0 * q):
#   x = fl(s dt), and the exponents fl(c x), fl(fl(-s c) T0) with c = fl(log2 e): three roundings
#     each, so an exponent of true size y is off by <= 3 y U and its exponential by the relative
#     3 y U; exp2 itself is good to one ulp = 2 U.                   E0: (3 s T0 + 2) U
#   x >= 0.05 (direct branch): e = exp2(..) carries (3 x + 2) U; omq = e; q = fl(1 - e) adds the
#     absolute e (3 x + 2) U (+ U q once e < 1/2), relative to q that is
#     e (3 x + 2) / (1 - e) + 1 <= 19.51 * 2.15 + 1 < 43 at x = 0.05, and falls with x.
#   x < 0.05 (polynomial): truncation x^4 / 120 < 0.9 U, the outer product and fma 2 U, the inner
#     fmas scaled by x, the argument 1 U: q within 4 U; omq = fl(1 - q) within 1.3 U.   Both < 43 U.
#   so  q: 43 U;  omq: (3 x + 2) U.   Then one rounding each for dt * omq, T0 * q, the difference
#   (relative to its result, <= |A| + |B|) and the final product:
#     A's share: (3 x + 2) + 1,  B's share: 43 + 1,  the difference 1,  E0 (3 s T0 + 2),  product 1
#   K = 43 + 1 + 1 + 2 + 1 = 48 covers both shares, and 3 s (T0 + dt) the two exponent terms.
K_ROUNDINGS = 48


def weight_bound(s, T0, dt):
    s = np.float64(np.float32(s))
    T0 = np.asarray(np.float32(T0), np.float64)
    dt = np.asarray(np.float32(dt), np.float64)
    q = -np.expm1(-s * dt)
    return (K_ROUNDINGS + 3.0 * s * (T0 + dt)) * U * np.exp(-s * T0) * (np.abs(dt * (1.0 - q)) + np.abs(T0 * q))


def fd_step(sigma):
    """h = 2^-12 * (the power of two at or below sigma): sigma +- h and sigma +- 2 h are exact in fp32."""
    h = 2.0 ** (np.floor(np.log2(float(sigma))) - 12)
    for m in (1, 2):
        for sg in (-1, 1):
            v = float(sigma) + sg * m * h
            assert float(np.float32(v)) == v, (sigma, h)
    return h


def fd_tangent(dose_at, sigma):
    """(T_h, T_2h): central differences of dose_at(sigma') (a float64 array) at sigma +- h and +- 2 h."""
    h = fd_step(sigma)
    T = []
    for m in (1, 2):
        T.append((np.asarray(dose_at(sigma + m * h), np.float64) - np.asarray(dose_at(sigma - m * h), np.float64))
                 / (2 * m * h))
    return T[0], T[1]


def assert_converged(T_h, T_2h):
    """The reference's own convergence: |T_h - T_2h| <= 1e-5 |T_h| (the truncation error scales as
    h^2, so T_h itself is then within ~3e-6 of the derivative)."""
    e = float(np.linalg.norm(T_h - T_2h)), float(np.linalg.norm(T_h))
    assert e[1] > 0 and e[0] <= 1e-5 * e[1], e
    return e[0] / e[1]


def film_errors(T, T_ref):
    """(relative L2, max |T - T_ref| / max |T_ref|)."""
    T, T_ref = np.asarray(T, np.float64), np.asarray(T_ref, np.float64)
    return (float(np.linalg.norm(T - T_ref) / np.linalg.norm(T_ref)),
            float(np.abs(T - T_ref).max() / np.abs(T_ref).max()))


def film_ok(T, T_ref):
    l2, mx = film_errors(T, T_ref)
    return l2 < RTOL and mx <= RTOL


def scalar_ok(g, G, T_ref):
    """|g - <G, T_ref>| <= 1e-4 <|G|, |T_ref|>."""
    G, T_ref = np.asarray(G, np.float64), np.asarray(T_ref, np.float64)
    return abs(float(g) - float(np.vdot(G, T_ref))) <= RTOL * float(np.vdot(np.abs(G), np.abs(T_ref)))


# --------------------------------------------------------------------------- a numpy stand-in renderer
class StandIn:
    """Rays through a 1-D row of voxels of pitch hx, for the checkers' self-tests.  Ray i enters the
    medium at o2 = -gap[i] before the grid (so the grid entry is at path length gap[i] > 0), runs
    along +x with direction cosine c[i] (visit length hx / c[i]) and carries the weight em[i].
    dose(s): float64.  tangent(s, defect): the fp32 weight of the library (host entry) per visit, with
    one deliberate defect:
      'grid_entry'  T0 measured from the grid entry instead of the segment origin
      'no_T0q'      the -T0 q term dropped
      'no_E0'       e^{-s T0} left out"""

    def __init__(self, n_rays=64, n_vox=37, hx=0.1, seed=0):
        rng = np.random.default_rng(seed)
        self.n_vox, self.hx = n_vox, hx
        self.gap = rng.uniform(0.2, 1.5, n_rays)
        self.c = rng.uniform(0.6, 1.0, n_rays)
        self.em = rng.uniform(0.0, 0.1, n_rays)
        self.first = rng.integers(0, 5, n_rays)

    def visits(self):
        for i in range(self.gap.size):
            dt = self.hx / self.c[i]
            v = np.arange(self.first[i], self.n_vox)
            T0 = self.gap[i] + dt * (v - self.first[i])
            yield i, v, T0, np.full(v.shape, dt)

    def dose(self, s):
        out = np.zeros(self.n_vox)
        for i, v, T0, dt in self.visits():
            np.add.at(out, v, self.em[i] * (np.exp(-s * T0) - np.exp(-s * (T0 + dt))))
        return out

    def tangent(self, s, defect=None):
        from drtvam_amd import _abi
        out = np.zeros(self.n_vox)
        for i, v, T0, dt in self.visits():
            if defect == "grid_entry":
                w = _abi.dsigma_weights(s, T0 - self.gap[i], dt).astype(np.float64)
            elif defect == "no_T0q":
                w = np.exp(-s * T0) * dt * np.exp(-s * dt)
            elif defect == "no_E0":
                w = _abi.dsigma_weights(s, T0, dt).astype(np.float64) * np.exp(s * T0)
            else:
                assert defect is None
                w = _abi.dsigma_weights(s, T0, dt).astype(np.float64)
            np.add.at(out, v, self.em[i] * w)
        return out


# --------------------------------------------------------------------------- scenes
def collimated_config(regular=True):
    """The config of projector_model.projector_scene('collimated', regular=regular), for the tests
    that need the scene itself (traverse / update) rather than its descriptor."""
    return {
        "vial": {"type": "index_matched", "r": 2.9, "height": 40.0,
                 "medium": {"ior": 1.0, "extinction": 1.0, "albedo": 0.0}},
        "projector": {"type": "collimated", "n_patterns": 6, "resx": 24, "resy": 20, "motion": "circular",
                      "distance": 20.0, "pixel_size": 0.15},
        "sensor": {"type": "dda", "scalex": 4.0, "scaley": 3.6, "scalez": 2.0,
                   "film": {"type": "vfilm", "resx": 36, "resy": 40, "resz": 20}},
        "target": {"analytic": "box_hole"},
        "loss": {"type": "threshold", "tl": 0.9, "tu": 0.95},
        "regular_sampling": regular,
    }


def with_sigma(desc, sigma):
    d = desc.copy()
    d.sigma_t = float(sigma)
    return d
