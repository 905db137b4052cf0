"""Float64 reference of fp_pose_errors (include/foundationpose_amd.h "pose errors"), from the inputs as given.

It shares no expression with the kernels: both point sets are taken to the CAMERA frame with the 4x4 matrices as they were passed
(no relative transform E^-1 G, no composites rounded to f32), the symmetries are conjugated as a product of three 4x4 matrices, the
rotation angle comes from the chord |R - I|_F = 2 sqrt(2) sin(theta / 2), and every mean is a plain float64 mean.

    ADD   = mean_v |E v - G v|                      ADD-S = mean_u min_v |G u - E v|
    MSSD  = min_s max_v |E v - G S'_s v|            MSPD  = min_s max_v |proj(E v) - proj(G S'_s v)|
    S'_s  = T(-c) S_s T(c)   (S_s in the mesh frame, v in the centred frame, c the mesh centre), S'_0 = I

over the vertices 0, step, 2 step, ... of the centred mesh (centred in f32, as the library stores it).

The bound the device is held to
-------------------------------
u = 2^-24 is the unit round-off of f32; r bounds |v| and |S'_s v| over the used vertices; tE = |t_E|, tG = |t_G|.

Paired kernel (ADD, MSSD).  A camera-space coordinate ((r0 x + r1 y) + r2 z) + t takes three products and three sums, so its error is
at most 4u (|r0 x| + |r1 y| + |r2 z| + |t|) <= 4u (sqrt(3) r + |t|) and the point's at most sqrt(3) times that:
    |fl(E v) - E v| <= u (12 r + 7 tE).
The composite G S'_s is formed in double and rounded once, each entry by a relative u: a further u (3 r + 2 (tG + r)) on b = (G S'_s) v,
whose translation is at most tG + r long:
    |fl(B v) - G S'_s v| <= u (12 r + 7 (tG + r)) + u (5 r + 2 tG) = u (24 r + 9 tG).
The three differences, three squares, two sums and the square root add at most 4u d with d <= tE + tG + 2 r.  Together
    |d_device - d| <= u (44 r + 13 (tE + tG)).

Nearest-neighbour kernel (ADD-S), in the relative frame D = E^-1 G: D is formed in double as (R_E^T R_G, R_E^T (t_G - t_E)) and rounded
once, the query is q = fl(D u), the targets v are exact.  The rounding of D costs u (3 r + 2 (tE + tG)), the transform u (12 r + 7 (tE + tG)).
R_E is a rotation rounded to f32, so R_E^T is its inverse up to 6u and E changes a length by at most 3u: that costs
6u (r + tE + tG) + 3u d.  The inner loop's squares, sums (fused or not) and the final root again at most 4u d.  Together
    |d_device - d| <= u (35 r + 22 (tE + tG)).
A minimum (a maximum) over v of values that are each off by at most b is off by at most b.

Both are below  POINT = u (48 r + 22 (tE + tG)),  which is what `metric_bound` uses.  A mean over Vs distances adds the quantum of the
integer sum, at most 2^-21 per term and so 2^-21 on the mean, and the final cast to f32, u times the mean:
    metric_bound = u (48 r + 22 (tE + tG)) + 2^-21 + u * value.
At the scale of the test cases (tE, tG <= 1 m, r <= 0.2 m) that is u * 53.6 + 2^-21 = 3.7e-6 m < 1e-5 m.

MSPD.  A projected coordinate is fx * (x / z) + cx, three f32 operations.  A camera-space error e moves it by at most
(fx / z)(1 + |x| / z) e, and the three roundings by at most 3u U, with U the largest |fx x / z| + |cx| (|fy y / z| + |cy|).  With
e_a + e_b <= u (36 r + 7 tE + 9 tG) from the paired kernel, rho = max(|x|, |y|) / z, two coordinates, and 4u on the final difference,
squares and root:
    pixel_bound = sqrt(2) ((f / z_min)(1 + rho) u (36 r + 9 (tE + tG)) + 6u U) + 4u * value.
"""
import numpy as np

f64 = np.float64
U = 2.0 ** -24
NEAR = float(np.float32(0.01))      # FP_RENDER_NEAR_M


def conjugated(symmetries, center):
    """[S + 1, 4, 4]: the identity, then T(-c) S_s T(c) for the mesh-frame symmetries"""
    c = np.asarray(center, f64)
    to_mesh, to_centred = np.eye(4), np.eye(4)
    to_mesh[:3, 3] = c
    to_centred[:3, 3] = -c
    out = [np.eye(4)]
    for s in np.asarray(symmetries if symmetries is not None else np.zeros((0, 4, 4)), f64).reshape(-1, 4, 4):
        out.append(to_centred @ s @ to_mesh)
    return np.stack(out)


def _apply(T, v):
    return v @ T[:3, :3].T + T[:3, 3]


def _project(K, p):
    return np.stack([K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2], K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2]], 1)


def nearest_mean(queries, targets, block=512):
    """mean over the queries of the distance to the nearest target"""
    best = np.empty(len(queries))
    for i in range(0, len(queries), block):
        d = queries[i:i + block, None, :] - targets[None, :, :]
        best[i:i + block] = np.sqrt((d * d).sum(-1)).min(1)
    return float(best.mean())


def rotation_angle_deg(R):
    """angle of the rotation nearest to R (a product of rotations that were rounded to f32 is one only up to ~3u) from its chord:
    |R - I|_F = 2 sqrt(2) sin(theta / 2), with cos(theta / 2) = sqrt((1 - s)(1 + s)) so that angles near 0 and near 180 are both exact"""
    a, _, bt = np.linalg.svd(R)
    s = min(1.0, np.linalg.norm(a @ bt - np.eye(3)) / (2.0 * np.sqrt(2.0)))
    return float(np.degrees(2.0 * np.arctan2(s, np.sqrt((1.0 - s) * (1.0 + s)))))


def pose_error(verts, center, K, E, G, symmetries=None, step=1, adds=True):
    """one record as a dict, float64; verts: the CENTRED vertices [V, 3] as the library stores them (f32)"""
    v = np.asarray(verts, f64)[::step]
    K, E, G = np.asarray(K, f64), np.asarray(E, f64), np.asarray(G, f64)
    a, g = _apply(E, v), _apply(G, v)
    rec = dict(n_vertices=len(v))
    rec["add_m"] = float(np.linalg.norm(a - g, axis=1).mean())
    rec["adds_m"] = nearest_mean(g, a) if adds else float("nan")
    near = bool((a[:, 2] < NEAR).any())
    surf, proj = [], []
    for S in conjugated(symmetries, center):
        b = _apply(G @ S, v)
        surf.append(np.linalg.norm(a - b, axis=1).max())
        near |= bool((b[:, 2] < NEAR).any())
        with np.errstate(all="ignore"):
            proj.append(np.linalg.norm(_project(K, a) - _project(K, b), axis=1).max())
    rec["per_sym_mssd"], rec["per_sym_mspd"] = np.array(surf), np.array(proj)
    rec["best_sym"] = int(np.argmin(surf))
    rec["mssd_m"] = float(surf[rec["best_sym"]])
    rec["best_sym_mspd"] = -1 if near else int(np.argmin(proj))
    rec["mspd_px"] = float("inf") if near else float(proj[rec["best_sym_mspd"]])
    GS = G @ conjugated(symmetries, center)[rec["best_sym"]]
    rec["rot_deg"] = rotation_angle_deg(E[:3, :3].T @ GS[:3, :3])
    rec["trans_m"] = float(np.linalg.norm(E[:3, 3] - GS[:3, 3]))
    # what the bounds need
    rec["r"] = float(max(np.linalg.norm(v, axis=1).max(), max(np.linalg.norm(_apply(S, v), axis=1).max() for S in conjugated(symmetries, center))))
    rec["tE"], rec["tG"] = float(np.linalg.norm(E[:3, 3])), float(np.linalg.norm(G[:3, 3]))
    if not near:
        pts = np.concatenate([a] + [_apply(G @ S, v) for S in conjugated(symmetries, center)])
        rec["z_min"] = float(pts[:, 2].min())
        rec["rho"] = float((np.abs(pts[:, :2]).max(1) / pts[:, 2]).max())
        rec["U"] = float(max((np.abs(K[0, 0] * pts[:, 0] / pts[:, 2]) + abs(K[0, 2])).max(), (np.abs(K[1, 1] * pts[:, 1] / pts[:, 2]) + abs(K[1, 2])).max()))
    return rec


def pose_errors(verts, center, K, est, gt, symmetries=None, step=1, adds=True):
    est, gt = np.asarray(est, f64).reshape(-1, 4, 4), np.asarray(gt, f64).reshape(-1, 4, 4)
    return [pose_error(verts, center, K, E, gt[0] if len(gt) == 1 else gt[i], symmetries, step, adds) for i, E in enumerate(est)]


def point_bound(r, tE, tG):
    return U * (48.0 * r + 22.0 * (tE + tG))


def metric_bound(rec, value):
    """metres: what |device - reference| of add_m, adds_m, mssd_m may be (module docstring)"""
    return point_bound(rec["r"], rec["tE"], rec["tG"]) + 2.0 ** -21 + U * abs(value)


def pixel_bound(rec, K, value):
    """pixels: the same for mspd_px"""
    f = max(abs(float(K[0][0])), abs(float(K[1][1])))
    e = U * (36.0 * rec["r"] + 9.0 * (rec["tE"] + rec["tG"]))
    return np.sqrt(2.0) * (f / rec["z_min"] * (1.0 + rec["rho"]) * e + 6.0 * U * rec["U"]) + 4.0 * U * abs(value)


# The host-derived fields are double arithmetic on f32 inputs, rounded once to f32: a relative 2^-23.  The angle also has an absolute
# floor: the matrices are rotations only up to the f32 rounding of their entries (each within 3u of a rotation, their product within 6u
# = 3.6e-7), and two well-conditioned angle formulas applied to such a matrix may differ by about twice that: 7.2e-7 rad = 4.1e-5 deg.
def angle_bound(value):
    return 5e-5 + 2.0 ** -22 * abs(value)      # degrees


def length_bound(value):
    return 1e-9 + 2.0 ** -22 * abs(value)
