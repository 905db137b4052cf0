"""References of fp_pose_vsd, shared by tests/test_vsd_ref_cpu.py and tests/test_vsd_gpu.py.

`counts` restates the section's per-pixel rules in numpy float32, operation by operation; `vsd` renders the two poses with
frame_render_ref.project / rasterize (the restatement of fp_render_pose the kernels are held to bit for bit) and calls it: this is what
the device record must EQUAL.

`intervals` is the float64 reference and shares no expression with either: it ray-casts the convex test shapes from the unsnapped
vertices, takes distances as |ray| * t, and says for every count the interval [certain, certain + uncertain] a correct implementation
must fall into.  A pixel is uncertain when its ray passes within the band visibility_ref.DELTA_FRAME (sqrt(2)/32 px of snapping plus the
f32 allowance) of the silhouette of either pose, or when one of the three comparisons (d - d_t against delta, |d_g - d_e| against a
threshold, D against 0.001) is within its band of the threshold: CMP_BAND for the observed depth, CMP_BAND plus the pixel's snap band
(see CMP_BAND) for a rendered distance.  The silhouette is a convex hull and a convex body has no occlusion contour inside it, so the
reference is for convex meshes only and says so (`is_convex`)."""
import numpy as np

import frame_render_ref as FR
from visibility_ref import DELTA_FRAME, SNAP

f32 = np.float32
MAX_TAUS = 16
# How far a rendered distance of the restatement may lie from the float64 ray-cast's, in metres, at one pixel:
#   * f32: the distance is z * q with z <= a few metres, a handful of roundings of 2^-24 each: below CMP_BAND = 1e-5 m.  This is all
#     that separates the two for the OBSERVED depth (D against 0.001, D * q).
#   * the 1/16 px snap: the rasteriser moves every vertex by at most SNAP = sqrt(2)/32 px on the screen, so the point of a facet seen at
#     a pixel is the one the unsnapped facet shows at most SNAP px away (a convex combination of three moves of at most SNAP), and the
#     distance changes by SNAP times the facet's slope |grad d| in metres per pixel.  With the ray r = ((u - cx)/fx, (v - cy)/fy, 1), the
#     facet's plane n . x = c and t = c / (n . r):  d = |r| t,  |grad t| = t sqrt((n_x/fx)^2 + (n_y/fy)^2) / |n . r|,  |grad |r|| <= 1/min(fx, fy),
#     so  |grad d| <= t / min(fx, fy) + |r| |grad t|.   A pixel within the snap of a facet's edge may be given the facet beyond it, whose
#     distance is continuous across the edge, so the slope of a pixel is the largest among its own facet and the facets that pass
#     within DELTA_FRAME px of it on the screen and within the bands of the surface there.  The slope is unbounded where
#     the surface turns edge-on, which on a convex body is the silhouette: those pixels are uncertain already (DELTA_FRAME), and what
#     the band admits elsewhere is counted: `intervals` returns the number of uncertain pixels, and its callers cap it.
# A constant band of 1e-5 m held for the 88 x 72 cases of tests/vsd_cases.py (f = 44 px at 0.3 m and more, facets leaning little) and
# failed under a general camera: at 0.13 m and f = 268 px one pixel is 5e-4 m wide, SNAP of it 2e-5 m, and a facet leaning 80 degrees
# moves by 1.2e-4 m (DESIGN.md section 4.11 has the numbers).
CMP_BAND = 1.0e-5   # metres
COUNTS = ("n_model_est", "n_model_gt", "n_visib_est", "n_visib_gt", "n_inter", "n_union")
EST_NEAR, EST_RANGE, GT_NEAR, GT_RANGE = 1, 2, 4, 8


# ---- the f32 restatement ----------------------------------------------------------------------------------------------------------------
def counts(z_e, z_g, D, K, delta, thr, wrong=None):
    """z_e, z_g: fp_render_pose's model_depth of the estimate and of the truth ([H,W] f32, 0 = background); D [H,W] f32 observed depth;
    thr: thresholds in metres -> dict of the six counts and n_fail [len(thr)].  wrong: a rule broken on purpose (negative controls):
    "no_vis_g_clause", "z_not_distance", "strict_threshold", "missing_hides"."""
    z_e, z_g, D = np.asarray(z_e, f32), np.asarray(z_g, f32), np.asarray(D, f32)
    H, W = D.shape
    K = np.asarray(K, f32).reshape(3, 3)
    delta = f32(delta)
    model_e, model_g = z_e != 0, z_g != 0
    X = (np.arange(W, dtype=f32)[None, :] - K[0, 2]) / K[0, 0]
    Y = (np.arange(H, dtype=f32)[:, None] - K[1, 2]) / K[1, 1]
    q = np.sqrt((X * X + Y * Y) + f32(1))
    if wrong == "z_not_distance":
        q = np.ones_like(q)
    assert q.dtype == f32
    with np.errstate(invalid="ignore"):
        d_t, d_e, d_g = D * q, z_e * q, z_g * q
        valid = np.ones_like(model_e) if wrong == "missing_hides" else ~(D < FR.MIN_DEPTH)
        hid_e, hid_g = valid & ((d_e - d_t) > delta), valid & ((d_g - d_t) > delta)
        vis_g = model_g & ~hid_g
        vis_e = model_e & ~hid_e if wrong == "no_vis_g_clause" else model_e & (~hid_e | vis_g)
        inter, union = vis_g & vis_e, vis_g | vis_e
        d = np.abs(d_g - d_e)
        fail = [inter & ((d > f32(t)) if wrong == "strict_threshold" else (d >= f32(t))) for t in thr]
    out = dict(n_model_est=int(model_e.sum()), n_model_gt=int(model_g.sum()), n_visib_est=int(vis_e.sum()), n_visib_gt=int(vis_g.sum()),
               n_inter=int(inter.sum()), n_union=int(union.sum()), n_fail=[int(f.sum()) for f in fail])
    return out


def thresholds(taus, diameter, normalized=True):
    """thr_t in metres: one f32 product with the diameter the model holds when normalised"""
    return [f32(t) * f32(diameter) if normalized else f32(t) for t in taus]


def host_vsd(n_fail, n_union, n_inter):
    """the record's vsd[t]: in double, rounded once"""
    return f32(1.0) if n_union == 0 else f32((float(n_fail) + float(n_union) - float(n_inter)) / float(n_union))


def record(c, status=0):
    """counts -> the record's fields: n_fail padded with 0 and vsd with NaN up to 16 entries; a refused pose has all counts 0 and vsd 1"""
    T = len(c["n_fail"])
    r = {k: (0 if status else c[k]) for k in COUNTS}
    r["n_fail"] = [0 if status else n for n in c["n_fail"]] + [0] * (MAX_TAUS - T)
    r["vsd"] = [host_vsd(r["n_fail"][t], r["n_union"], r["n_inter"]) for t in range(T)] + [f32(np.nan)] * (MAX_TAUS - T)
    r["status"] = status
    return r


def model_depth(verts, faces, pose, K, H, W):
    """fp_render_pose's model_depth [H,W] f32 of centred vertices under pose, or the refusal bits (1 near, 2 range) of a refused pose"""
    cam, snap, near, far = FR.project(verts, pose, K)
    if near.any() or far.any():
        return (1 if near.any() else 0) | (2 if far.any() else 0)
    keys = FR.rasterize(cam, snap, FR.stored_faces(verts, faces), H, W)
    return np.where(keys != FR.EMPTY, (keys >> np.uint64(32)).astype(np.uint32).view(f32), f32(0)).astype(f32)


def vsd(mesh, est, gt, D, K, delta=0.015, taus=(0.2,), normalized=True, wrong=None):
    """records of est [N,4,4] against gt ([N,4,4] or [1,4,4]) on the depth D: what fp_pose_vsd must return, field for field"""
    est, gt = np.asarray(est, f32).reshape(-1, 4, 4), np.asarray(gt, f32).reshape(-1, 4, 4)
    D = np.asarray(D, f32)
    H, W = D.shape
    verts = FR.centred(mesh)
    thr = thresholds(taus, mesh.diameter, normalized)
    planes = {}

    def plane(pose):
        key = pose.tobytes()
        if key not in planes:
            planes[key] = model_depth(verts, mesh.faces, pose, K, H, W)
        return planes[key]

    empty = dict({k: 0 for k in COUNTS}, n_fail=[0] * len(thr))
    out = []
    for i, E in enumerate(est):
        ze, zg = plane(E), plane(gt[i if len(gt) > 1 else 0])
        status = (ze if isinstance(ze, int) else 0) | ((zg if isinstance(zg, int) else 0) << 2)
        out.append(record(empty, status) if status else record(counts(ze, zg, D, K, delta, thr, wrong)))
    return out


# ---- the float64 reference --------------------------------------------------------------------------------------------------------------
def _hull(p):
    """convex hull of points [n,2], counter-clockwise in (x, y)"""
    p = sorted(set(map(tuple, p)))

    def half(points):
        h = []
        for q in points:
            while len(h) >= 2 and (h[-1][0] - h[-2][0]) * (q[1] - h[-2][1]) - (h[-1][1] - h[-2][1]) * (q[0] - h[-2][0]) <= 0:
                h.pop()
            h.append(q)
        return h

    lo, up = half(p), half(p[::-1])
    return np.array(lo[:-1] + up[:-1], np.float64)


def is_convex(mesh, eps=1e-9):
    """every vertex lies on one side of every face's plane (to eps metres), the same side for all faces"""
    v = (np.asarray(mesh.vertices, f32) - np.asarray(mesh.center, f32)).astype(np.float64)
    f = np.asarray(mesh.faces, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    keep = np.linalg.norm(n, axis=1) > 0
    n, f = n[keep] / np.linalg.norm(n[keep], axis=1, keepdims=True), f[keep]
    side = np.einsum("fvk,fk->fv", v[None, :, :] - v[f[:, 0]][:, None, :], n)
    return bool((side <= eps).all() or (side >= -eps).all())


def _cast(mesh, pose, K, H, W):
    """-> (inside [H,W] bool: the pixel's ray meets the body, edge [H,W]: distance in px to its silhouette, dist [H,W]: |ray| * t of the
    nearest intersection, inf where none, band [H,W]: the snap band of dist in metres (see CMP_BAND), 0 where none)"""
    v = (np.asarray(mesh.vertices, f32) - np.asarray(mesh.center, f32)).astype(np.float64)
    P = np.asarray(np.asarray(pose, f32), np.float64)
    K = np.asarray(np.asarray(K, f32), np.float64).reshape(3, 3)
    cam = v @ P[:3, :3].T + P[:3, 3]
    assert (cam[:, 2] > 0.02).all(), "the float64 reference is for poses well in front of the camera"
    uv = np.stack([K[0, 0] * cam[:, 0] / cam[:, 2] + K[0, 2], K[1, 1] * cam[:, 1] / cam[:, 2] + K[1, 2]], 1)
    hull = _hull(uv)
    nxt = np.roll(hull, -1, 0)
    cc, rr = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    s = np.stack([cc, rr], -1)[:, :, None, :]                                # [H,W,1,2]
    e = (nxt - hull)[None, None]
    rel = s - hull[None, None]
    side = e[..., 0] * rel[..., 1] - e[..., 1] * rel[..., 0]                 # > 0 on the inner side of every edge of a ccw hull
    t = np.clip((rel * e).sum(-1) / (e * e).sum(-1), 0.0, 1.0)
    edge = np.linalg.norm(rel - t[..., None] * e, axis=-1).min(-1)
    inside = (side > 0).all(-1)
    # nearest intersection of the ray lambda * (X, Y, 1) with any triangle, over the window of the triangle's bounding box (every vertex
    # is in front of the camera, so a ray outside the box of the three projected corners cannot meet the triangle)
    ray = np.stack([(cc - K[0, 2]) / K[0, 0], (rr - K[1, 2]) / K[1, 1], np.ones_like(cc)], -1)
    length = np.linalg.norm(ray, axis=-1)
    best = np.full((H, W), np.inf)
    own = np.zeros((H, W))                                                   # |grad dist| in metres per pixel, of the facet that wins
    faces = np.asarray(mesh.faces, np.int64)

    def window(q):
        c0, r0 = np.maximum(np.floor(q.min(0)).astype(np.int64) - 1, 0)
        c1, r1 = np.minimum(np.ceil(q.max(0)).astype(np.int64) + 1, [W - 1, H - 1])
        return None if c0 > c1 or r0 > r1 else (slice(r0, r1 + 1), slice(c0, c1 + 1))

    def plane(a, b, c, win):
        n = np.cross(b - a, c - a)
        den = ray[win] @ n
        lam = (a @ n) / den
        return n, lam, lam / min(K[0, 0], K[1, 1]) + length[win] * lam * np.hypot(n[0] / K[0, 0], n[1] / K[1, 1]) / np.abs(den)

    for (a, b, c), q in zip(cam[faces], uv[faces]):
        win = window(q)
        if win is None:
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            n, lam, lean = plane(a, b, c, win)
            hit = lam[..., None] * ray[win]
            ok = np.isfinite(lam) & (lam > 0)
            for p0, p1 in ((a, b), (b, c), (c, a)):
                ok &= (np.cross(p1 - p0, hit - p0) @ n) >= -1e-12 * (n @ n)
            wins = ok & (lam < best[win])
        best[win] = np.where(wins, lam, best[win])
        own[win] = np.where(wins, lean, own[win])
    dist = length * best
    # a pixel within the snap of a facet's edge may be given the facet beyond it: the steepest of the facets that pass within
    # DELTA_FRAME px of the pixel on the screen and, there, within both bands of the surface
    steepest = own.copy()
    for (a, b, c), q in zip(cam[faces], uv[faces]):
        win = window(q)
        if win is None:
            continue
        p = np.stack([cc[win], rr[win]], -1)
        e = np.roll(q, -1, 0) - q                                            # [3,2]
        rel = p[..., None, :] - q                                            # [h,w,3,2]
        cross = e[:, 0] * rel[..., 1] - e[:, 1] * rel[..., 0]
        within = (cross >= 0).all(-1) | (cross <= 0).all(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            along = np.clip((rel * e).sum(-1) / (e * e).sum(-1), 0.0, 1.0)
            apart = np.where(within, 0.0, np.nan_to_num(np.linalg.norm(rel - along[..., None] * e, axis=-1), nan=np.inf).min(-1))
            _, lam, lean = plane(a, b, c, win)
            near = (apart <= DELTA_FRAME) & np.isfinite(lam) & (lam > 0) & np.isfinite(best[win])
            near &= length[win] * np.abs(lam - np.where(np.isfinite(best[win]), best[win], 0.0)) <= DELTA_FRAME * (lean + own[win]) + CMP_BAND
        steepest[win] = np.where(near & (lean > steepest[win]), lean, steepest[win])
    return inside, edge, dist, np.where(np.isfinite(dist), SNAP * steepest, 0.0)


def intervals(mesh, E, G, D, K, delta=0.015, taus=(0.2,), normalized=True, snap_band=True):
    """one pose pair of a CONVEX mesh -> ({count: (lo, hi)} with n_fail a list of pairs, n_uncertain).  snap_band=False: the constant
    band of 1e-5 m alone, as before the snap band was derived (tests/test_camera_cases_cpu.py shows that it is too narrow)"""
    assert is_convex(mesh), "the float64 reference takes the convex hull for the silhouette and knows no inner occlusion contour"
    D = np.asarray(np.asarray(D, f32), np.float64)
    H, W = D.shape
    thr = [float(f32(t)) * float(f32(mesh.diameter)) if normalized else float(f32(t)) for t in taus]
    in_e, edge_e, dist_e, band_e = _cast(mesh, E, K, H, W)
    in_g, edge_g, dist_g, band_g = _cast(mesh, G, K, H, W)
    if not snap_band:
        band_e, band_g = 0.0, 0.0
    Kd = np.asarray(np.asarray(K, f32), np.float64).reshape(3, 3)
    cc, rr = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    norm = np.sqrt(((cc - Kd[0, 2]) / Kd[0, 0]) ** 2 + ((rr - Kd[1, 2]) / Kd[1, 1]) ** 2 + 1.0)
    dist_t = norm * D
    unsure = (edge_e <= DELTA_FRAME) | (edge_g <= DELTA_FRAME)
    unsure |= (in_e & ~np.isfinite(dist_e)) | (in_g & ~np.isfinite(dist_g))          # (a ray that slipped between two triangles)
    with np.errstate(invalid="ignore"):
        covered = in_e | in_g
        unsure |= covered & (np.abs(D - 0.001) <= CMP_BAND)
        valid = ~(D < 0.001)
        gap_e, gap_g = dist_e - dist_t - delta, dist_g - dist_t - delta
        unsure |= in_e & valid & (np.abs(gap_e) <= CMP_BAND + band_e)
        unsure |= in_g & valid & (np.abs(gap_g) <= CMP_BAND + band_g)
        vis_g = in_g & ~(valid & (gap_g > 0))
        vis_e = in_e & (~(valid & (gap_e > 0)) | vis_g)
        both = in_e & in_g
        diff = np.abs(np.where(both, dist_g, 0.0) - np.where(both, dist_e, 0.0))
        for t in thr:
            unsure |= both & (np.abs(diff - t) <= CMP_BAND + band_e + band_g)
    sure = ~unsure
    inter, union = vis_g & vis_e, vis_g | vis_e
    n_unsure = int(unsure.sum())

    def span(mask):
        lo = int((mask & sure).sum())
        return lo, lo + n_unsure

    out = dict(n_model_est=span(in_e), n_model_gt=span(in_g), n_visib_est=span(vis_e), n_visib_gt=span(vis_g), n_inter=span(inter),
               n_union=span(union), n_fail=[span(inter & (diff >= t)) for t in thr])
    return out, n_unsure


def inside(rec, iv):
    """names of the counts of record `rec` that fall outside their interval"""
    bad = [k for k in COUNTS if not iv[k][0] <= rec[k] <= iv[k][1]]
    bad += [f"n_fail[{t}]" for t, (lo, hi) in enumerate(iv["n_fail"]) if not lo <= rec["n_fail"][t] <= hi]
    return bad
