"""References of fp_pose_search and fp_register_depth, shared by tests/test_search_ref_cpu.py and the GPU tests.

(a) `records` restates the section's per-point rules in numpy float32, operation by operation (np.rint, the same association order, the
same float comparisons): the ten integers of a device record must EQUAL it.

(b) `records64` is the float64 restatement and shares no expression with (a): plain vector algebra, floor(x + 0.5) for the pixel (checked
to agree with rint away from ties), facing by an actual angle.  `compare` counts the (pose, step, point) triples the two classify
differently.

`register_ref` is steps 2 to 5 of fp_register_depth on top of (a); the hypothesis poses and the ICP are arguments."""
import numpy as np

import frame_render_ref as FR
import icp_ref as IR

f32 = np.float32
NEAR = f32(0.01)               # FP_RENDER_NEAR_M
MIN_DEPTH = f32(0.001)
MIN_COS2 = f32(0.04)
MAX_POINTS, MAX_STEPS = 4096, 64
REFUSED_NEAR = 1
FIELDS = ("n_facing", "n_inlier", "n_front", "n_behind", "n_outside", "n_missing", "score", "best_step", "n_points", "status")
# classes of a (pose, step, point): 0 not facing, then the five counted ones
NOT_FACING, INLIER, FRONT, BEHIND, OUTSIDE, MISSING = range(6)
WRONG = ("step_direction", "no_facing_test", "ge_for_gt", "half_pixel")


def normals_of(mesh):
    return np.ascontiguousarray(mesh.normals, f32)


def smallest_step(V, cap=1024):
    return max((V + cap - 1) // cap, 1)


# ---- (a) the f32 restatement ------------------------------------------------------------------------------------------------------------
def classify(verts, normals, poses, K, D, n_steps, step_m, tol_m, vertex_step=1, wrong=None):
    """verts: CENTRED vertices [V,3]; normals [V,3] as loaded; poses [N,4,4] (numpy, row-major); D [H,W] f32 raw depth ->
    (cls [N, n_steps, P] of the classes above, refused [N, n_steps]).  wrong: a rule broken on purpose (negative controls), one of WRONG."""
    assert wrong is None or wrong in WRONG
    p = np.asarray(verts, f32)[::vertex_step]
    n = np.asarray(normals, f32)[::vertex_step]
    T = np.asarray(poses, f32).reshape(-1, 4, 4)
    K = np.asarray(K, f32).reshape(3, 3)
    D = np.asarray(D, f32)
    H, W = D.shape
    step, tol = f32(step_m), f32(tol_m)
    R = T[:, :3, :3]

    def rot(v):    # [N, P, 3]: ((r0 x + r1 y) + r2 z), row by row
        return np.stack([(R[:, i, 0, None] * v[None, :, 0] + R[:, i, 1, None] * v[None, :, 1]) + R[:, i, 2, None] * v[None, :, 2] for i in range(3)], -1)

    rp, rn = rot(p), rot(n)
    assert rp.dtype == f32 and rn.dtype == f32
    t = T[:, :3, 3]
    s = np.arange(n_steps).astype(f32) * step                                        # [K]
    if wrong == "step_direction":
        s = -s
    with np.errstate(all="ignore"):
        tk = np.stack([t[:, 0, None] + s[None, :] * (t[:, 0] / t[:, 2])[:, None], t[:, 1, None] + s[None, :] * (t[:, 1] / t[:, 2])[:, None],
                       t[:, 2, None] + s[None, :]], -1)                              # [N, K, 3]
        q = rp[:, None, :, :] + tk[:, :, None, :]                                    # [N, K, P, 3]
        qx, qy, qz = q[..., 0], q[..., 1], q[..., 2]
        refused = (qz < NEAR).any(-1)
        m = rn[:, None, :, :]
        a = -((m[..., 0] * qx + m[..., 1] * qy) + m[..., 2] * qz)
        facing = (a > 0) & (a * a > MIN_COS2 * ((qx * qx + qy * qy) + qz * qz))
        if wrong == "no_facing_test":
            facing = np.ones_like(facing)
        u = K[0, 0] * (qx / qz) + K[0, 2]
        v = K[1, 1] * (qy / qz) + K[1, 2]
        uf, vf = (np.floor(u), np.floor(v)) if wrong == "half_pixel" else (np.rint(u), np.rint(v))
        inside = (uf >= 0) & (uf <= f32(W - 1)) & (vf >= 0) & (vf <= f32(H - 1))
        assert a.dtype == f32 and u.dtype == f32 and uf.dtype == f32
        ui = np.where(inside, uf, 0).astype(np.int64)
        vi = np.where(inside, vf, 0).astype(np.int64)
        Dp = D[vi, ui]
        seen = (Dp >= MIN_DEPTH) & np.isfinite(Dp)
        dz = Dp - qz
        assert dz.dtype == f32
        inl = np.abs(dz) <= tol
        front = dz < -tol
        behind = dz >= tol if wrong == "ge_for_gt" else dz > tol
    cls = np.select([~facing, ~inside, ~seen, behind, front, inl], [NOT_FACING, OUTSIDE, MISSING, BEHIND, FRONT, INLIER], MISSING).astype(np.int8)
    return cls, refused


def summarise(cls, refused):
    """-> the records of classify's output: a list of dicts with FIELDS"""
    out = []
    for c, r in zip(cls, refused):
        counts = np.stack([(c == k).sum(-1) for k in (INLIER, FRONT, BEHIND, OUTSIDE, MISSING)], -1).astype(np.int64)      # [K, 5]
        score = counts[:, 0] - counts[:, 2] - counts[:, 3]
        rec = dict.fromkeys(FIELDS, 0)
        rec["n_points"] = int(c.shape[-1])
        if r.all():
            rec["best_step"], rec["status"] = -1, REFUSED_NEAR
        else:
            k = int(np.argmax(np.where(r, np.iinfo(np.int64).min, score)))           # (the first maximum: the lowest step on ties)
            rec.update(n_facing=int(counts[k].sum()), n_inlier=int(counts[k, 0]), n_front=int(counts[k, 1]), n_behind=int(counts[k, 2]),
                       n_outside=int(counts[k, 3]), n_missing=int(counts[k, 4]), score=int(score[k]), best_step=k)
        out.append(rec)
    return out


def records(verts, normals, poses, K, D, n_steps, step_m, tol_m, vertex_step=1, wrong=None):
    return summarise(*classify(verts, normals, poses, K, D, n_steps, step_m, tol_m, vertex_step, wrong))


def at_step(pose, k, step_m):
    """the pose moved to its step k: t_k in f32"""
    P = np.array(pose, f32)
    s = f32(k) * f32(step_m)
    t = P[:3, 3].copy()
    P[0, 3] = t[0] + s * (t[0] / t[2])
    P[1, 3] = t[1] + s * (t[1] / t[2])
    P[2, 3] = t[2] + s
    return P


# ---- (b) the float64 restatement --------------------------------------------------------------------------------------------------------
def classify64(verts, normals, poses, K, D, n_steps, step_m, tol_m, vertex_step=1):
    """-> (cls, refused) like classify, in float64 and by other means"""
    pts = np.asarray(np.asarray(verts, f32), np.float64)[::vertex_step]
    nrm = np.asarray(np.asarray(normals, f32), np.float64)[::vertex_step]
    T = np.asarray(np.asarray(poses, f32), np.float64).reshape(-1, 4, 4)
    Kd = np.asarray(np.asarray(K, f32), np.float64).reshape(3, 3)
    D = np.asarray(D, f32)
    H, W = D.shape
    limit = np.arccos(0.2)
    cls = np.zeros((len(T), n_steps, len(pts)), np.int8)
    refused = np.zeros((len(T), n_steps), bool)
    for i, P in enumerate(T):
        origin = P[:3, 3]
        along = origin / origin[2]                                                   # the ray of the origin, one metre of z per unit
        world_n = nrm @ P[:3, :3].T
        for k in range(n_steps):
            cam = pts @ P[:3, :3].T + (origin + float(f32(k) * f32(step_m)) * along)
            refused[i, k] = bool((cam[:, 2] < float(NEAR)).any())
            with np.errstate(all="ignore"):
                cosine = -(world_n * cam).sum(1) / np.linalg.norm(cam, axis=1)
                angle = np.arccos(np.clip(cosine, -1, 1))
                facing = angle < limit
                pix = (Kd @ (cam / cam[:, 2:3]).T).T[:, :2]
                cell = np.floor(pix + 0.5)
                away = np.abs(pix - np.floor(pix) - 0.5) > 1e-9
                assert (cell[away] == np.rint(pix[away])).all()                      # floor(x + 0.5) is rint away from ties
                inside = (cell[:, 0] >= 0) & (cell[:, 0] < W) & (cell[:, 1] >= 0) & (cell[:, 1] < H)
                col = np.where(inside, cell[:, 0], 0).astype(np.int64)
                row = np.where(inside, cell[:, 1], 0).astype(np.int64)
                obs = D[row, col].astype(np.float64)
                known = np.isfinite(obs) & (obs >= float(MIN_DEPTH))
                gap = obs - cam[:, 2]
            c = np.full(len(pts), INLIER, np.int8)
            c[gap > float(f32(tol_m))] = BEHIND
            c[gap < -float(f32(tol_m))] = FRONT
            c[~known] = MISSING
            c[~inside] = OUTSIDE
            c[~facing] = NOT_FACING
            cls[i, k] = c
    return cls, refused


def compare(verts, normals, poses, K, D, n_steps, step_m, tol_m, vertex_step=1, wrong=None):
    """(a), possibly with a broken rule, against (b) -> dict(n_facing: triples either calls facing, n_diff: triples the two classify
    differently, refused_equal)"""
    ca, ra = classify(verts, normals, poses, K, D, n_steps, step_m, tol_m, vertex_step, wrong)
    cb, rb = classify64(verts, normals, poses, K, D, n_steps, step_m, tol_m, vertex_step)
    live = ~(ra | rb)[:, :, None]
    return dict(n_facing=int((((ca != NOT_FACING) | (cb != NOT_FACING)) & live).sum()), n_diff=int(((ca != cb) & live).sum()),
                refused_equal=bool((ra == rb).all()))


# ---- steps 2 to 5 of fp_register_depth --------------------------------------------------------------------------------------------------
def pick_candidates(recs, top_k):
    """step 3: indices of the top_k records by score, ties to the lower index, refused poses dropped"""
    ok = [i for i, r in enumerate(recs) if r["status"] == 0]
    return sorted(ok, key=lambda i: (-recs[i]["score"], i))[:top_k]


def pick_winner(cands, refined):
    """step 5: cands [hypothesis index], refined [dict(status, n_used, n_behind, e2)] -> position in cands, or None"""
    alive = [c for c in range(len(cands)) if not refined[c]["status"] & (IR.REFUSED_NEAR | IR.REFUSED_RANGE | IR.TOO_FEW)]
    if not alive:
        return None
    return min(alive, key=lambda c: (-(refined[c]["n_used"] - refined[c]["n_behind"]), refined[c]["e2"], cands[c]))


def register_ref(mesh, hyp_poses, K, D, icp, top_k=16, tol_m=0.005, iterations=15):
    """hyp_poses [N,4,4]; icp: IR.icp32 or IR.icp64 -> dict(pose, hypothesis, n_candidates, rank_key, search, candidates: [(hypothesis,
    start pose, icp result)]), or None when no candidate is left"""
    verts = FR.centred(mesh)
    step_m = f32(mesh.diameter) / f32(16)
    recs = records(verts, normals_of(mesh), hyp_poses, K, D, 9, step_m, tol_m, smallest_step(len(verts)))
    cands = pick_candidates(recs, top_k)
    gate = float(min(f32(4) * f32(tol_m), f32(mesh.diameter)))
    runs, brief = [], []
    for i in cands:
        start = at_step(hyp_poses[i], recs[i]["best_step"], step_m)
        res = icp(mesh, start, K, D, gate, iterations)
        last = res["last"]
        runs.append((i, start, res))
        brief.append(dict(status=res["status"], n_used=last["n_used"], n_behind=last["n_behind"], e2=last["sums"][27] if "sums" in last else last["e2"]))
    w = pick_winner(cands, brief)
    if w is None:
        return None
    return dict(pose=np.asarray(runs[w][2]["pose"]), hypothesis=cands[w], n_candidates=len(cands), rank_key=brief[w]["n_used"] - brief[w]["n_behind"],
                search=recs[cands[w]], candidates=runs, searched=recs)
