"""References of fp_refine_depth, shared by tests/test_icp_ref_cpu.py and the GPU tests.

(a) `sums` restates the section's per-pixel rules in numpy float32, operation by operation, on top of frame_render_ref's rasteriser (the
restatement of fp_render_pose the kernels are held to bit for bit): the six counts and the 28 integer sums the device record must EQUAL.

(b) `icp64` is the float64 reference and shares no expression with (a): it ray-casts the mesh from the unsnapped float64 vertices, forms
J and e with vector algebra, sums in float64, solves with numpy.linalg.eigh and iterates with the section's stopping rules.

`compare` holds one evaluation of (a) to one of (b): the pixels the two classify differently (or see another triangle of) are counted,
and A and b must agree within `bounds`, which is derived from u = 2^-24, the 2^-33 quantum and the 1/16 px snap (see there)."""
import numpy as np

import frame_render_ref as FR

f32 = np.float32
MIN_COS = f32(0.2)
MIN_PIXELS = 32
EPS_ROT, EPS_TRANS = float(f32(1e-5)), float(f32(1e-6))
RANK_EPS = 1e-8
Q32 = f32(2.0 ** 32)
CONVERGED, TOO_FEW, REFUSED_NEAR, REFUSED_RANGE = 1, 2, 4, 8
COUNTS = ("n_model", "n_valid", "n_used", "n_front", "n_behind", "n_grazing")
# classes of a pixel: 0 no model, 1 used, 2 front, 3 behind, 4 grazing, 5 model without a valid depth
NONE, USED, FRONT, BEHIND, GRAZING, INVALID = range(6)
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]


# ---- (a) the f32 restatement ------------------------------------------------------------------------------------------------------------
def sums(verts, faces, pose, K, D, max_dist, diameter, wrong=None, maps=False):
    """verts: CENTRED vertices; pose 4x4 (numpy, row-major); D [H,W] f32 raw depth -> dict(counts..., sums=[28 ints]) or the refusal
    bits (REFUSED_NEAR / REFUSED_RANGE) of a pose fp_render_pose refuses.  wrong: a rule broken on purpose (negative controls):
    "sign_of_e", "t_not_subtracted", "gate_on_dz", "normal_not_normalised".  maps: also cls [H,W] and tri [H,W]."""
    P = np.asarray(pose, f32)
    K = np.asarray(K, f32).reshape(3, 3)
    D = np.asarray(D, f32)
    H, W = D.shape
    cam, snap, near, far = FR.project(verts, P, K)
    if near.any() or far.any():
        return (REFUSED_NEAR if near.any() else 0) | (REFUSED_RANGE if far.any() else 0)
    fs = FR.stored_faces(verts, faces)
    keys = FR.rasterize(cam, snap, fs, H, W)
    model = keys != FR.EMPTY
    rr, cc = np.nonzero(model)
    z = (keys[model] >> np.uint64(32)).astype(np.uint32).view(f32)
    tri = (keys[model] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    f = fs[tri]
    p0, p1, p2 = cam[f[:, 0]], cam[f[:, 1]], cam[f[:, 2]]
    a, b = p1 - p0, p2 - p0
    nx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    ny = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    nz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    len2 = (nx * nx + ny * ny) + nz * nz
    flat = ~(len2 > 0)
    with np.errstate(all="ignore"):
        ln = np.sqrt(len2)
        if wrong == "normal_not_normalised":
            ln = np.ones_like(ln)
        hx, hy, hz = (np.where(flat, f32(0), n / ln).astype(f32) for n in (nx, ny, nz))
        X = (cc.astype(f32) - K[0, 2]) / K[0, 0]
        Y = (rr.astype(f32) - K[1, 2]) / K[1, 1]
        l = np.sqrt((X * X + Y * Y) + f32(1))
        s = (hx * X + hy * Y) + hz
        Dp = D[rr, cc]
        valid = (Dp >= FR.MIN_DEPTH) & np.isfinite(Dp)
        dz = Dp - z
        along = dz if wrong == "gate_on_dz" else dz * l
        gate = f32(max_dist)
        front = valid & (along < -gate)
        behind = valid & ~front & (along > gate)
        grazing = valid & ~front & ~behind & (np.abs(s) / l < MIN_COS)
        used = valid & ~front & ~behind & ~grazing
        rad = f32(diameter) * f32(0.5)
        e = (dz * s) / rad
        if wrong == "sign_of_e":
            e = -e
        t = np.zeros(3, f32) if wrong == "t_not_subtracted" else P[:3, 3]
        qx, qy, qz = Dp * X, Dp * Y, Dp
        cx, cy, cz = (qx - t[0]) / rad, (qy - t[1]) / rad, (qz - t[2]) / rad
        J = [cy * hz - cz * hy, cz * hx - cx * hz, cx * hy - cy * hx, hx, hy, hz]
        assert all(v.dtype == f32 for v in J + [e, l, s, along])

        def q32(v):
            return int(np.rint(v[used] * Q32).astype(np.int64).sum())

        out = dict(n_model=int(model.sum()), n_valid=int(valid.sum()), n_used=int(used.sum()), n_front=int(front.sum()),
                   n_behind=int(behind.sum()), n_grazing=int(grazing.sum()),
                   sums=[q32(J[i] * J[j]) for i, j in PAIRS] + [q32(J[i] * e) for i in range(6)] + [q32(e * e)])
    if maps:
        cls = np.zeros((H, W), np.int64)
        cls[rr, cc] = np.select([used, front, behind, grazing], [USED, FRONT, BEHIND, GRAZING], INVALID)
        tmap = np.full((H, W), -1, np.int64)
        tmap[rr, cc] = tri
        out["cls"], out["tri"] = cls, tmap
    return out


def rms_m(sums28, n_used, diameter):
    """the record's rms_m: in double, rounded once"""
    return f32(0) if n_used == 0 else f32(np.sqrt(float(sums28[27]) / 4294967296.0 / float(n_used)) * float(f32(diameter) * f32(0.5)))


def system(sums28):
    """-> (A [6,6], b [6]) in float64 from the 28 integers"""
    A = np.zeros((6, 6))
    for k, (i, j) in enumerate(PAIRS):
        A[i, j] = A[j, i] = sums28[k] / 4294967296.0
    return A, np.array(sums28[21:27], np.float64) / 4294967296.0


# ---- (b) the float64 reference ----------------------------------------------------------------------------------------------------------
def _cast64(cam, faces, K, H, W):
    """nearest intersection of every pixel's ray (X, Y, 1) with the triangles cam[faces] -> (z [H,W], inf where none; tri [H,W], -1)"""
    faces = np.asarray(faces, np.int64)
    tri = cam[faces]                                                              # [F,3,3]
    uv = np.stack([K[0, 0] * tri[..., 0] / tri[..., 2] + K[0, 2], K[1, 1] * tri[..., 1] / tri[..., 2] + K[1, 2]], -1)
    lo = np.maximum(np.floor(uv.min(1)).astype(np.int64) - 1, 0)
    hi = np.minimum(np.ceil(uv.max(1)).astype(np.int64) + 1, [W - 1, H - 1])
    best = np.full(H * W, np.inf)
    win = np.full(H * W, -1, np.int64)
    size = (hi - lo + 1).max(1)
    seen = (hi >= lo).all(1)
    small = seen & (size <= 12)
    groups = [np.nonzero(small)[0]] + [np.array([k]) for k in np.nonzero(seen & ~small)[0]]
    hits = []
    for g in groups:
        if len(g) == 0:
            continue
        m = int(size[g].max())
        px = lo[g, 0][:, None, None] + np.arange(m)[None, None, :] + np.zeros((1, m, 1), np.int64)
        py = lo[g, 1][:, None, None] + np.arange(m)[None, :, None] + np.zeros((1, 1, m), np.int64)
        ok = (px <= hi[g, 0][:, None, None]) & (py <= hi[g, 1][:, None, None])
        ray = np.stack([(px - K[0, 2]) / K[0, 0], (py - K[1, 2]) / K[1, 1], np.ones(px.shape)], -1)      # [G,m,m,3]
        a, b, c = tri[g, 0], tri[g, 1], tri[g, 2]
        n = np.cross(b - a, c - a)
        nn = (n * n).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            lam = ((a * n).sum(-1) / nn)[:, None, None] / ((ray * n[:, None, None, :]).sum(-1) / nn[:, None, None])
            hit = lam[..., None] * ray
            ok &= np.isfinite(lam) & (lam > 0) & (nn > 0)[:, None, None]
            for p, q in ((a, b), (b, c), (c, a)):
                side = (np.cross((q - p)[:, None, None, :], hit - p[:, None, None, :]) * n[:, None, None, :]).sum(-1)
                ok &= side >= -1e-12 * nn[:, None, None]
        idx = (py * W + px)[ok]
        hits.append((idx, lam[ok], np.broadcast_to(g[:, None, None], ok.shape)[ok]))
    if hits:
        idx, lam, who = (np.concatenate(x) for x in zip(*hits))
        np.minimum.at(best, idx, lam)
        first = lam == best[idx]
        win[idx[first]] = who[first]
    return best.reshape(H, W), win.reshape(H, W)


def evaluate64(mesh, pose, K, D, max_dist):
    """one evaluation in float64 -> dict(A, b, e2, counts..., cls [H,W], tri [H,W])"""
    v = (np.asarray(mesh.vertices, f32) - np.asarray(mesh.center, f32)).astype(np.float64)
    P = np.asarray(pose, np.float64)
    K = np.asarray(np.asarray(K, f32), np.float64).reshape(3, 3)
    D = np.asarray(np.asarray(D, f32), np.float64)
    H, W = D.shape
    cam = v @ P[:3, :3].T + P[:3, 3]
    assert (cam[:, 2] > 0.02).all(), "the float64 reference is for poses well in front of the camera"
    faces = np.asarray(mesh.faces, np.int64)
    z, win = _cast64(cam, faces, K, H, W)
    model = win >= 0
    rr, cc = np.nonzero(model)
    t3 = cam[faces[win[model]]]
    normal = np.cross(t3[:, 1] - t3[:, 0], t3[:, 2] - t3[:, 0])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    ray = np.stack([(cc - K[0, 2]) / K[0, 0], (rr - K[1, 2]) / K[1, 1], np.ones(len(cc))], 1)
    length = np.linalg.norm(ray, axis=1)
    cosine = (normal * ray).sum(1)
    obs = D[model]
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(obs) & (obs >= float(FR.MIN_DEPTH))
        gap = (obs - z[model]) * length
        front, behind = valid & (gap < -max_dist), valid & (gap > max_dist)
        grazing = valid & ~front & ~behind & (np.abs(cosine) < float(MIN_COS) * length)
    used = valid & ~front & ~behind & ~grazing
    half = float(f32(mesh.diameter)) / 2
    point = obs[used, None] * ray[used]
    resid = ((point - z[model][used, None] * ray[used]) * normal[used]).sum(1) / half          # n . (q - p) / rad
    Jm = np.concatenate([np.cross((point - P[:3, 3]) / half, normal[used]), normal[used]], 1)
    cls = np.zeros((H, W), np.int64)
    cls[rr, cc] = np.select([used, front, behind, grazing], [USED, FRONT, BEHIND, GRAZING], INVALID)
    return dict(A=Jm.T @ Jm, b=Jm.T @ resid, e2=float(resid @ resid), n_model=int(model.sum()), n_valid=int(valid.sum()), n_used=int(used.sum()),
                n_front=int(front.sum()), n_behind=int(behind.sum()), n_grazing=int(grazing.sum()), cls=cls, tri=win)


def solve64(A, b, translation_only=False):
    """-> (xi [6], rank, lambda_min / lambda_max) with numpy.linalg.eigh; directions below RANK_EPS * lambda_max do not move"""
    o = 3 if translation_only else 0
    w, v = np.linalg.eigh(A[o:, o:])
    xi = np.zeros(6)
    if not w.max() > 0:
        return xi, 0, 0.0
    keep = w >= RANK_EPS * w.max()
    xi[o:] = v[:, keep] @ ((v[:, keep].T @ b[o:]) / w[keep])
    return xi, int(keep.sum()), float(w.min() / w.max())


def twist(pose, xi, half):
    """R <- exp(omega) R, t <- t + upsilon (upsilon = xi[3:] * half): the twist about the object's origin"""
    w = xi[:3]
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    E = np.eye(3) + Kx + Kx @ Kx / 2 if th < 1e-9 else np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * (Kx @ Kx)
    out = np.array(pose, np.float64)
    out[:3, :3] = E @ out[:3, :3]
    out[:3, 3] += xi[3:] * half
    return out


def icp64(mesh, pose, K, D, max_dist, iterations, translation_only=False):
    """the float64 ICP -> dict(pose [4,4] f64, status, iterations, rank, cond, steps [(rot_rad, trans_m, cond)], last: the last evaluation)"""
    half = float(f32(mesh.diameter)) / 2
    P = np.asarray(np.asarray(pose, f32), np.float64)
    out = dict(status=0, iterations=0, rank=0, cond=0.0, steps=[])
    fill = False
    for k in range(iterations + 1):
        ev = evaluate64(mesh, P, K, D, max_dist)
        out["last"] = ev
        if fill or k == iterations:
            break
        if ev["n_used"] < MIN_PIXELS:
            out["status"] |= TOO_FEW
            break
        xi, out["rank"], out["cond"] = solve64(ev["A"], ev["b"], translation_only)
        rot, trans = float(np.linalg.norm(xi[:3])), float(np.linalg.norm(xi[3:]) * half)
        out["steps"].append((rot, trans, out["cond"]))
        P = twist(P, xi, half)
        out["iterations"] += 1
        if rot < EPS_ROT and trans < EPS_TRANS:
            out["status"] |= CONVERGED
            fill = True
    out["pose"] = P
    return out


# ---- (a) against (b) --------------------------------------------------------------------------------------------------------------------
def pose_gap(P, Q):
    """-> (degrees, metres) between two poses"""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    c = (np.trace(P[:3, :3] @ Q[:3, :3].T) - 1) / 2
    return float(np.degrees(np.arccos(np.clip(c, -1, 1)))), float(np.linalg.norm(P[:3, 3] - Q[:3, 3]))


def bounds(mesh, pose, K, max_dist, n_same, n_diff):
    """how far A and b of (a) may lie from (b)'s, per entry, on n_same pixels both use with the same triangle plus n_diff pixels they
    treat differently.  Per pixel, with u = 2^-24, z_max the farthest vertex, f the focal length, r_max the largest vertex norm:
      * a used pixel has |q - p| <= max_dist, so |qc| <= c_q = (r_max + max_dist) / rad (at least 1), |J_i| <= c_q, |e| <= c_e = max_dist / rad;
      * a corner difference p1 - p0 carries 4 u z_max of rounding, so the unit normal is off by d_n = 8 u z_max / edge_min + 8 u;
      * J = (qc x n, n): d_J = c_q d_n + 16 u;
      * the rasteriser's vertices are snapped by at most sqrt(2)/32 px = (sqrt(2)/32) z_max / f metres across the ray; on a used pixel
        the surface leans at most atan(sqrt(1 / 0.2^2 - 1)) from the ray, so z moves by d_z = 4.9 (sqrt(2)/32) z_max / f, plus 16 u z_max
        of rounding in the perspective-correct depth;
      * e = dz s / rad: d_e = (d_z + max_dist 2 d_n) / rad + 8 u;
      * a product of two such values is off by |x| d_y + |y| d_x, plus the 2^-33 quantum of its integer.
    A pixel only one of them uses, or with another triangle, may differ by the whole term: 2 c_q^2 in A, 2 c_q c_e in b."""
    u = 2.0 ** -24
    v = (np.asarray(mesh.vertices, f32) - np.asarray(mesh.center, f32)).astype(np.float64)
    P = np.asarray(pose, np.float64)
    z_max = float((v @ P[:3, :3].T + P[:3, 3])[:, 2].max())
    f = np.asarray(mesh.faces, np.int64)
    edges = np.concatenate([np.linalg.norm(v[f[:, i]] - v[f[:, (i + 1) % 3]], axis=1) for i in range(3)])
    Kd = np.asarray(K, np.float64).reshape(3, 3)
    focal = float(min(Kd[0, 0], Kd[1, 1]))
    half = float(f32(mesh.diameter)) / 2
    c_q = max((float(np.linalg.norm(v, axis=1).max()) + max_dist) / half, 1.0)
    c_e = max_dist / half
    d_n = 8 * u * z_max / float(edges[edges > 0].min()) + 8 * u
    d_J = c_q * d_n + 16 * u
    d_z = 4.9 * (np.sqrt(2) / 32) * z_max / focal + 16 * u * z_max
    d_e = (d_z + max_dist * 2 * d_n) / half + 8 * u
    bound_A = n_same * (2 * c_q * d_J + 2.0 ** -33) + n_diff * 2 * c_q * c_q
    bound_b = n_same * (c_q * d_e + c_e * d_J + 2.0 ** -33) + n_diff * 2 * c_q * c_e
    return bound_A, bound_b


def compare(mesh, pose, K, D, max_dist, wrong=None):
    """one evaluation of (a) against (b) -> dict(n_model, n_diff: pixels of another class or triangle, dA, db: largest entry differences,
    bound_A, bound_b)"""
    a = sums(FR.centred(mesh), mesh.faces, pose, K, D, max_dist, mesh.diameter, wrong=wrong, maps=True)
    b = evaluate64(mesh, pose, K, D, max_dist)
    A, bb = system(a["sums"])
    ca, cb = a["cls"], b["cls"]
    # (frame_render_ref.stored_faces keeps the order of the faces, so the triangle ids are comparable)
    diff = (ca != cb) | (((ca == USED) | (cb == USED)) & (a["tri"] != b["tri"]))
    n_same = int(((ca == USED) & (cb == USED) & ~diff).sum())
    bound_A, bound_b = bounds(mesh, pose, K, max_dist, n_same, int(diff.sum()))
    return dict(n_model=max(a["n_model"], b["n_model"]), n_class=int((ca != cb).sum()), n_diff=int(diff.sum()), dA=float(np.abs(A - b["A"]).max()),
                db=float(np.abs(bb - b["b"]).max()), bound_A=bound_A, bound_b=bound_b, a=a, b=b)


def icp32(mesh, pose, K, D, max_dist, iterations, translation_only=False):
    """the iteration as the library runs it, on (a)'s integer sums: the pose is kept in double and rounded to f32 for every evaluation ->
    dict(pose [4,4] f32, status, iterations, steps, last: the last evaluation of (a)).  For poses fp_render_pose does not refuse."""
    half = float(f32(mesh.diameter) * f32(0.5))
    verts = FR.centred(mesh)
    P = np.asarray(np.asarray(pose, f32), np.float64)
    out = dict(status=0, iterations=0, rank=0, cond=0.0, steps=[])
    fill = False
    for k in range(iterations + 1):
        ev = sums(verts, mesh.faces, P.astype(f32), K, D, max_dist, mesh.diameter)
        out["last"] = ev
        if fill or k == iterations:
            break
        if ev["n_used"] < MIN_PIXELS:
            out["status"] |= TOO_FEW
            break
        A, b = system(ev["sums"])
        xi, out["rank"], out["cond"] = solve64(A, b, translation_only)
        rot, trans = float(np.linalg.norm(xi[:3])), float(np.linalg.norm(xi[3:]) * half)
        out["steps"].append((rot, trans, out["cond"]))
        before = P.astype(f32)
        P = twist(P, xi, half)
        out["iterations"] += 1
        if rot < EPS_ROT and trans < EPS_TRANS:
            out["status"] |= CONVERGED
            fill = True
            if P.astype(f32).tobytes() == before.tobytes():
                break
    out["pose"] = P.astype(f32)
    return out
