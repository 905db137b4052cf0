"""References of fp_refine_silhouette, shared by tests/test_silref_ref_cpu.py and the GPU tests.

(a) `sums` restates the section's rules in numpy float32, operation by operation, on top of frame_render_ref's rasteriser and
silhouette_ref's brute-force distance maps: the seven counts and the 28 integer sums the device record must EQUAL.

(b) `evaluate64` is the float64 reference and shares no expression with (a): it ray-casts the mesh from the unsnapped float64 vertices
(icp_ref's caster), finds the outline with a padded minimum filter, measures the distance of a pixel to the mask's outline by brute force
over pixel centres, and forms J by central finite differences of the projected contour point under the six twist generators.

`compare` holds one evaluation of (a) to one of (b): every pixel the two classify differently must lie on or beside a pixel whose
coverage the 1/16 px snap can change, and A and b must agree entry-wise within `bounds`, which is derived from u = 2^-24, the 2^-25
quantum and the 1/16 px snap (see there).

`silref32` is the iteration as the library runs it (step cap, stops), on (a)'s integer sums."""
import numpy as np

import frame_render_ref as FR
import icp_ref as IR
import silhouette_ref as SR

f32 = np.float32
MAX_TERM = f32(64.0)
MAX_STEP_RAD, MAX_STEP_RADII = 0.2, 0.5
MIN_PIXELS = 16
MAX_ITERATIONS = 32
EPS_ROT, EPS_TRANS = IR.EPS_ROT, IR.EPS_TRANS
Q24 = f32(2.0 ** 24)
CONVERGED, TOO_FEW, REFUSED_NEAR, REFUSED_RANGE = 1, 2, 4, 8
TRANSLATION_ONLY, OCCLUSION = 1, 2
COUNTS = ("n_model", "n_contour", "n_used", "n_occluded", "n_far", "n_flat", "n_steep")
INTS = COUNTS + ("iterations", "rank", "status")
FLOATS = ("rms_px", "scale_px", "cond", "last_rot_rad", "last_trans_m", "reserved_f")
# classes of a pixel: 0 no contour pixel, 1 used, 2 occluded, 3 far, 4 flat, 5 steep
NONE, USED, OCCLUDED, FAR, FLAT, STEEP = range(6)
PAIRS = IR.PAIRS
WRONG = ("outside_is_background", "eight_neighbours", "gradient_not_halved", "sign_of_e", "t_not_subtracted", "psi_without_the_one")


# ---- (a) the f32 restatement ------------------------------------------------------------------------------------------------------------
def signed_map(mask, d2=None):
    """sd [H,W] int64: -d2_to_bg on a mask pixel, d2_to_mask elsewhere"""
    on = np.asarray(mask) > 0
    d2m, d2b = SR.maps(mask) if d2 is None else d2
    return np.where(on, -d2b, d2m).astype(np.int64)


def psi32(sd, wrong=None):
    sd = np.asarray(sd, np.int64)
    one = f32(0) if wrong == "psi_without_the_one" else f32(1)
    with np.errstate(invalid="ignore"):
        pos = np.sqrt(np.maximum(sd, 0).astype(f32))
        neg = one - np.sqrt(np.maximum(-sd, 0).astype(f32))
    return np.where(sd > 0, pos, np.where(sd == 0, f32(0), neg)).astype(f32)


def pose_constants(P, K, diameter):
    """(rad, s, kx, ky) in f32, or None for a pose with !(t.z >= FP_RENDER_NEAR_M)"""
    P, K = np.asarray(P, f32), np.asarray(K, f32).reshape(3, 3)
    rad = f32(diameter) * f32(0.5)
    if not P[2, 3] >= FR.NEAR:
        return None
    s = (K[0, 0] * rad) / P[2, 3]
    return rad, s, (K[0, 0] * rad) / s, (K[1, 1] * rad) / s


def sums(verts, faces, pose, K, sd, diameter, D=None, gate_px=0, tol=0.005, occlusion=False, wrong=None, maps=False, only=None):
    """verts: CENTRED vertices; pose 4x4 (numpy, row-major); sd: signed_map(mask); D [H,W] f32 raw depth, read with `occlusion` only ->
    dict(counts..., sums=[28 ints], scale_px) or the refusal bits of a pose that is refused.  wrong: a rule broken on purpose (WRONG).
    maps: also cls [H,W], tri [H,W] and model [H,W].  only [H,W] bool: the 28 sums run over the used pixels inside it (the counts do not change)."""
    P = np.asarray(pose, f32)
    K = np.asarray(K, f32).reshape(3, 3)
    sd = np.asarray(sd, np.int64)
    H, W = sd.shape
    cam, snap, near, far = FR.project(verts, P, K)
    consts = pose_constants(P, K, diameter)
    if near.any() or far.any() or consts is None:
        return (REFUSED_NEAR if near.any() or consts is None else 0) | (REFUSED_RANGE if far.any() else 0)
    rad, s, kx, ky = consts
    fs = FR.stored_faces(verts, faces)
    keys = FR.rasterize(cam, snap, fs, H, W)
    model = keys != FR.EMPTY
    # a neighbour that is not a model pixel; one outside the frame does not count
    pad = np.pad(model, 1, constant_values=(wrong != "outside_is_background"))
    bare = ~pad[1:-1, :-2] | ~pad[1:-1, 2:] | ~pad[:-2, 1:-1] | ~pad[2:, 1:-1]
    if wrong == "eight_neighbours":
        bare |= ~pad[:-2, :-2] | ~pad[:-2, 2:] | ~pad[2:, :-2] | ~pad[2:, 2:]
    contour = model & bare
    rr, cc = np.nonzero(contour)
    z = (keys[contour] >> np.uint64(32)).astype(np.uint32).view(f32)
    tri = (keys[contour] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    s0 = sd[rr, cc]
    with np.errstate(all="ignore"):
        if occlusion:
            Dp = np.asarray(D, f32)[rr, cc]
            occluded = ~(Dp < FR.MIN_DEPTH) & (Dp < z - f32(tol))
        else:
            occluded = np.zeros(len(rr), bool)
        far_px = ~occluded & (gate_px > 0) & (np.abs(s0) > gate_px * gate_px)
        psi = psi32(s0, wrong)
        half = f32(1.0) if wrong == "gradient_not_halved" else f32(0.5)
        gx = (psi32(sd[rr, np.minimum(cc + 1, W - 1)], wrong) - psi32(sd[rr, np.maximum(cc - 1, 0)], wrong)) * half
        gy = (psi32(sd[np.minimum(rr + 1, H - 1), cc], wrong) - psi32(sd[np.maximum(rr - 1, 0), cc], wrong)) * half
        flat = ~occluded & ~far_px & (gx == 0) & (gy == 0)
        X = (cc.astype(f32) - K[0, 2]) / K[0, 0]
        Y = (rr.astype(f32) - K[1, 2]) / K[1, 1]
        ax, ay = (gx * kx) / z, (gy * ky) / z
        az = -(ax * X + ay * Y)
        t = np.zeros(3, f32) if wrong == "t_not_subtracted" else P[:3, 3]
        px, py, pz = (z * X - t[0]) / rad, (z * Y - t[1]) / rad, (z - t[2]) / rad
        J = [py * az - pz * ay, pz * ax - px * az, px * ay - py * ax, ax, ay, az]
        e = -psi / s
        if wrong == "sign_of_e":
            e = -e
        assert all(v.dtype == f32 for v in J + [e, psi, gx, gy])
        small = np.abs(e) <= MAX_TERM
        for v in J:
            small &= np.abs(v) <= MAX_TERM
        steep = ~occluded & ~far_px & ~flat & ~small
        used = ~occluded & ~far_px & ~flat & small

        summed = used if only is None else used & np.asarray(only, bool)[rr, cc]

        def q24(v):
            return int(np.rint(v[summed] * Q24).astype(np.int64).sum())

        out = dict(n_model=int(model.sum()), n_contour=len(rr), n_used=int(used.sum()), n_occluded=int(occluded.sum()), n_far=int(far_px.sum()),
                   n_flat=int(flat.sum()), n_steep=int(steep.sum()), scale_px=s,
                   sums=[q24(J[i] * J[j]) for i, j in PAIRS] + [q24(J[i] * e) for i in range(6)] + [q24(e * e)])
    if maps:
        cls = np.zeros((H, W), np.int64)
        cls[rr, cc] = np.select([used, occluded, far_px, flat], [USED, OCCLUDED, FAR, FLAT], STEEP)
        tmap = np.full((H, W), -1, np.int64)
        tmap[rr, cc] = tri
        out.update(cls=cls, tri=tmap, model=model, psi=dict(zip(zip(rr.tolist(), cc.tolist()), psi.tolist())))
    return out


def rms_px(sums28, n_used, scale_px):
    """the record's rms_px: in double, rounded once"""
    return f32(0) if n_used == 0 else f32(np.sqrt(float(sums28[27]) / 16777216.0 / float(n_used)) * float(scale_px))


def system(sums28):
    """-> (A [6,6], b [6]) in float64 from the 28 integers"""
    A = np.zeros((6, 6))
    for k, (i, j) in enumerate(PAIRS):
        A[i, j] = A[j, i] = sums28[k] / 16777216.0
    return A, np.array(sums28[21:27], np.float64) / 16777216.0


def capped(xi):
    """the step cap: the whole twist scaled by min(1, MAX_STEP_RAD / |omega|, MAX_STEP_RADII / |upsilon|) -> (xi, scale)"""
    rot, radii = float(np.linalg.norm(xi[:3])), float(np.linalg.norm(xi[3:]))
    scale = 1.0
    if rot > MAX_STEP_RAD:
        scale = min(scale, MAX_STEP_RAD / rot)
    if radii > MAX_STEP_RADII:
        scale = min(scale, MAX_STEP_RADII / radii)
    return (xi * scale if scale < 1.0 else xi), scale


def silref32(mesh, pose, K, mask, iterations, gate_px=0, tol=0.005, translation_only=False, occlusion=False, D=None, sd=None):
    """the iteration as the library runs it, on (a)'s integer sums: the pose is kept in double and rounded to f32 for every evaluation ->
    dict(pose [4,4] f32, status, iterations, rank, cond, steps [(rot, trans, scale)], last: the last evaluation of (a) at the returned pose)"""
    half = float(f32(mesh.diameter) * f32(0.5))
    verts = FR.centred(mesh)
    sd = signed_map(mask) if sd is None else sd
    P = np.asarray(np.asarray(pose, f32), np.float64)
    out = dict(status=0, iterations=0, rank=0, cond=0.0, steps=[], last=None)
    fill = False
    for k in range(iterations + 1):
        ev = sums(verts, mesh.faces, P.astype(f32), K, sd, mesh.diameter, D=D, gate_px=gate_px, tol=tol, occlusion=occlusion)
        if isinstance(ev, int):                       # refused: at the input the pose stays, after an update it goes back
            out["status"] |= ev
            if k > 0:
                P = P_prev
                out["iterations"] -= 1
            break
        out["last"] = ev
        if fill or k == iterations:
            break
        if ev["n_used"] < MIN_PIXELS:
            out["status"] |= TOO_FEW
            break
        A, b = system(ev["sums"])
        xi, out["rank"], out["cond"] = IR.solve64(A, b, translation_only)
        rot, trans = float(np.linalg.norm(xi[:3])), float(np.linalg.norm(xi[3:]) * half)
        xi, scale = capped(xi)
        out["steps"].append((rot, trans, scale))
        P_prev = P
        P = IR.twist(P, xi, half)
        out["iterations"] += 1
        if rot < EPS_ROT and trans < EPS_TRANS:
            out["status"] |= CONVERGED
            fill = True
            if P.astype(f32).tobytes() == P_prev.astype(f32).tobytes():
                break
    out["pose"] = P.astype(f32)
    return out


# ---- (b) the float64 reference ----------------------------------------------------------------------------------------------------------
def _outline_distance(on, rr, cc):
    """float64 distance in pixels from the pixel centres (rr, cc) to the mask's outline, by brute force over pixel centres: outside the
    mask the distance to the nearest mask pixel, inside one minus the distance to the nearest pixel that is none"""
    mr, mc = np.nonzero(on)
    br, bc = np.nonzero(~on)
    out = np.empty(len(rr))
    for i, (r, c) in enumerate(zip(rr, cc)):
        if on[r, c]:
            out[i] = 1.0 - np.sqrt(((br - r) ** 2 + (bc - c) ** 2).min())
        else:
            out[i] = np.sqrt(((mr - r) ** 2 + (mc - c) ** 2).min())
    return out


def _rodrigues(w):
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + Kx if th == 0 else np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * (Kx @ Kx)


def evaluate64(mesh, pose, K, mask, gate_px=0):
    """one evaluation in float64 (no occlusion) -> dict(A, b, e2, counts..., cls [H,W], tri [H,W], model [H,W], and per used pixel, in
    row-major order of the frame: J [n,6], e [n], lean [n] = |grad z| in metres per pixel of the winning triangle's plane, z [n])"""
    v = (np.asarray(mesh.vertices, f32) - np.asarray(mesh.center, f32)).astype(np.float64)
    P = np.asarray(pose, np.float64)
    K = np.asarray(np.asarray(K, f32), np.float64).reshape(3, 3)
    on = np.asarray(mask) > 0
    H, W = on.shape
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    R, t = P[:3, :3], P[:3, 3]
    cam = v @ R.T + t
    assert (cam[:, 2] > 0.02).all(), "the float64 reference is for poses well in front of the camera"
    faces = np.asarray(mesh.faces, np.int64)
    depth, win = IR._cast64(cam, faces, K, H, W)
    model = win >= 0
    # outline: the smallest of the four neighbours' coverage, the frame's surroundings counted as covered
    pad = np.pad(model.astype(np.int64), 1, constant_values=1)
    least = np.minimum(np.minimum(pad[1:-1, :-2], pad[1:-1, 2:]), np.minimum(pad[:-2, 1:-1], pad[2:, 1:-1]))
    contour = model & (least == 0)
    rr, cc = np.nonzero(contour)
    half = float(f32(mesh.diameter)) / 2
    scale = fx * half / t[2]
    d0 = _outline_distance(on, rr, cc)
    east = _outline_distance(on, rr, np.minimum(cc + 1, W - 1))
    west = _outline_distance(on, rr, np.maximum(cc - 1, 0))
    south = _outline_distance(on, np.minimum(rr + 1, H - 1), cc)
    north = _outline_distance(on, np.maximum(rr - 1, 0), cc)
    grad = np.stack([(east - west) / 2, (south - north) / 2], 1)
    beyond = np.where(d0 > 0, d0, 1.0 - d0)                       # the distance the gate is about: to the other side
    far_px = (gate_px > 0) & (beyond > gate_px + 1e-9)
    flat = ~far_px & (grad == 0).all(1)
    point = depth[contour][:, None] * np.stack([(cc - cx) / fx, (rr - cy) / fy, np.ones(len(cc))], 1)

    def projected(p):
        return np.stack([fx * p[:, 0] / p[:, 2] + cx, fy * p[:, 1] / p[:, 2] + cy], 1)

    h = 1e-5
    Jm = np.zeros((len(rr), 6))
    for k in range(6):
        g = np.zeros(6)
        g[k] = h
        moved = [(point - t) @ _rodrigues(sgn * g[:3]).T + t + sgn * g[3:] * half for sgn in (1.0, -1.0)]
        flow = (projected(moved[0]) - projected(moved[1])) / (2 * h)          # pixels per unit of the twist (radians, radii)
        Jm[:, k] = (grad * flow).sum(1) / scale
    resid = -d0 / scale
    steep = ~far_px & ~flat & ((np.abs(Jm) > float(MAX_TERM)).any(1) | (np.abs(resid) > float(MAX_TERM)))
    used = ~far_px & ~flat & ~steep
    t3 = cam[faces[win[contour]]]
    normal = np.cross(t3[:, 1] - t3[:, 0], t3[:, 2] - t3[:, 0])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    ray = point / point[:, 2:3]
    with np.errstate(divide="ignore"):
        lean = point[:, 2] * np.hypot(normal[:, 0] / fx, normal[:, 1] / fy) / np.abs((normal * ray).sum(1))
    cls = np.zeros((H, W), np.int64)
    cls[rr, cc] = np.select([used, far_px, flat], [USED, FAR, FLAT], STEEP)
    Ju, eu = Jm[used], resid[used]
    return dict(A=Ju.T @ Ju, b=Ju.T @ eu, e2=float(eu @ eu), n_model=int(model.sum()), n_contour=len(rr), n_used=int(used.sum()), n_occluded=0,
                n_far=int(far_px.sum()), n_flat=int(flat.sum()), n_steep=int(steep.sum()), cls=cls, tri=win, model=model, J=Ju, e=eu, lean=lean[used],
                z=point[used, 2], rr=rr[used], cc=cc[used], grad=grad[used], scale_px=scale, cam=cam)


# ---- (a) against (b) --------------------------------------------------------------------------------------------------------------------
SNAP_PX = np.sqrt(2.0) / 32                       # how far the 1/16 px snap moves a projected vertex, at most


def unsure_pixels(cam, faces, K, H, W):
    """[H,W] bool: the pixels whose centre lies within SNAP_PX (and 1e-6 px of rounding) of a projected triangle edge: the snap can move
    the edge across the centre, so the pixel's coverage, or the triangle that wins it, may differ between (a) and (b)"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    uv = np.stack([K[0, 0] * cam[:, 0] / cam[:, 2] + K[0, 2], K[1, 1] * cam[:, 1] / cam[:, 2] + K[1, 2]], 1)
    f = np.asarray(faces, np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    p = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64)
    out = np.zeros(H * W, bool)
    seen = set()
    for tri in f:
        for i in range(3):
            a, b = int(tri[i]), int(tri[(i + 1) % 3])
            if (min(a, b), max(a, b)) in seen:
                continue
            seen.add((min(a, b), max(a, b)))
            d = uv[b] - uv[a]
            n2 = float(d @ d)
            lam = np.clip(((p - uv[a]) @ d) / n2, 0, 1) if n2 > 0 else np.zeros(len(p))
            out |= np.linalg.norm(p - (uv[a] + lam[:, None] * d), axis=1) <= SNAP_PX + 1e-6
    return out.reshape(H, W)


def bounds(b, K, half, t, same):
    """how far A and b of (a) may lie from (b)'s, per entry, both summed over the pixels both use with the same triangle (`same`, a mask
    over (b)'s used pixels): the sum of a per-pixel bound.  With u = 2^-24:
      * psi and its gradient are functions of integers: (a)'s carry 2 u |psi| and 4 u of rounding, nothing else;
      * the snap moves the projected corners of the winning triangle by SNAP_PX at most while their depths stay, so the depth of the plane
        at the pixel moves by d_z = 2 lean SNAP_PX (lean = |grad z| per pixel of the plane; twice the first-order term), plus 16 u z
        of rounding in the perspective-correct depth;
      * a = g k / z: d_a = |a| (d_z / z + 8 u);  a_z = -(a_x X + a_y Y) inherits it: |a| below is the norm of all three;
      * pc = (z ray - t) / rad: d_p = (d_z |ray| + 8 u (z |ray| + |t|)) / rad;
      * J = (pc x a, a): d_J = 2 (|pc| d_a + |a| d_p) + 16 u |pc| |a| for the first three, d_a for the others (the larger is used for all);
      * e = -psi / s does not depend on z: d_e = 8 u |e|;
      * a product of two such values is off by |x| d_y + |y| d_x, plus the 2^-25 quantum of its integer; the finite differences of (b)
        (h = 1e-5) add 1e-8 to every J."""
    u = 2.0 ** -24
    K = np.asarray(K, np.float64).reshape(3, 3)
    J, e, z, lean = b["J"][same], b["e"][same], b["z"][same], b["lean"][same]
    ray = np.stack([(b["cc"][same] - K[0, 2]) / K[0, 0], (b["rr"][same] - K[1, 2]) / K[1, 1], np.ones(int(same.sum()))], 1)
    L = np.linalg.norm(ray, axis=1)
    a = np.linalg.norm(J[:, 3:], axis=1)
    pc = np.linalg.norm((z[:, None] * ray - t) / half, axis=1)
    d_z = 2 * lean * SNAP_PX + 16 * u * z
    d_a = a * (d_z / z + 8 * u)
    d_p = (d_z * L + 8 * u * (z * L + np.linalg.norm(t))) / half
    d_J = np.maximum(2 * (pc * d_a + a * d_p) + 16 * u * pc * a, d_a) + 1e-8
    d_e = 8 * u * np.abs(e)
    Jmax = np.abs(J).max(axis=1) + d_J
    bound_A = float((2 * Jmax * d_J + 2.0 ** -25).sum())
    bound_b = float((Jmax * d_e + (np.abs(e) + d_e) * d_J + 2.0 ** -25).sum())
    return bound_A, bound_b


def compare(mesh, pose, K, mask, gate_px=0, wrong=None, sd=None):
    """one evaluation of (a) against (b) -> dict(n_class: pixels of another class, n_diff: pixels of another class or triangle,
    n_unexplained: those of them that neither are nor touch a pixel the snap can change (must be 0), dA, db: largest entry differences of
    the two systems summed over the pixels both use with the same triangle, bound_A, bound_b)"""
    sd = signed_map(mask) if sd is None else sd
    a = sums(FR.centred(mesh), mesh.faces, pose, K, sd, mesh.diameter, gate_px=gate_px, wrong=wrong, maps=True)
    b = evaluate64(mesh, pose, K, mask, gate_px=gate_px)
    H, W = sd.shape
    ca, cb = a["cls"], b["cls"]
    unsure = unsure_pixels(b["cam"], mesh.faces, K, H, W)
    pad = np.pad(unsure, 1)
    beside = unsure | pad[1:-1, :-2] | pad[1:-1, 2:] | pad[:-2, 1:-1] | pad[2:, 1:-1]
    differ = ca != cb
    # (frame_render_ref.stored_faces keeps the order of the faces, so the triangle ids are comparable)
    diff = differ | (((ca == USED) | (cb == USED)) & (a["tri"] != b["tri"]))
    same = ~diff[b["rr"], b["cc"]]
    half = float(f32(mesh.diameter)) / 2
    bound_A, bound_b = bounds(b, K, half, np.asarray(pose, np.float64)[:3, 3], same)
    A, bb = system(sums(FR.centred(mesh), mesh.faces, pose, K, sd, mesh.diameter, gate_px=gate_px, wrong=wrong, only=(ca == USED) & (cb == USED) & ~diff)["sums"])
    Js, es = b["J"][same], b["e"][same]
    return dict(n_contour=max(a["n_contour"], b["n_contour"]), n_same=int(same.sum()), n_class=int(differ.sum()), n_diff=int(diff.sum()),
                n_unexplained=int((diff & ~beside).sum()), dA=float(np.abs(A - Js.T @ Js).max()), db=float(np.abs(bb - Js.T @ es).max()),
                bound_A=bound_A, bound_b=bound_b, a=a, b=b)
