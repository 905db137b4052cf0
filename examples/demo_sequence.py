#!/usr/bin/env python3
"""Python twin of examples/fp_demo.cpp: Register the first frame, Track the rest, write poses.txt + box overlays.

    python examples/demo_sequence.py --data test_data/mustard0 --refiner refiner.fpw --scorer scorer.fpw --out out
    python examples/demo_sequence.py --synthetic 8 --out out      # seeded synthetic sequence + synthetic weights; its ground truth also
                                                                  # gives out/errors.txt (ADD, ADD-S, MSSD, MSPD per frame) and the two AUCs
    python examples/demo_sequence.py --synthetic 8 --fit 5        # + pose-fit columns (tolerance 5 mm) and a LOST? marker per frame
    python examples/demo_sequence.py --synthetic 8 --depth-filter # the networks see bilateral(erode(depth)), like FoundationPose as published
    python examples/demo_sequence.py --synthetic 8 --render       # + <id>_render.png beside every box plot: the model's visible pixels, flat-shaded over the frame
    python examples/demo_sequence.py --synthetic 8 --no-weights   # no networks: fp_register_depth on the first frame, fp_refine_depth from the previous
                                                                  # answer on the others; with --synthetic the error against the scene's truth per frame
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundationpose_cpp_amd import FoundationPose, _lib, auc, dataset as D, load_mesh, weights as W  # noqa: E402
from foundationpose_cpp_amd.synthetic import to_colmajor  # noqa: E402


def run(data, refiner, scorer, out, name="mustard", refine_itr=1, plots=False, fit_mm=None, lost_below=0.5, depth_filter=False, render=False,
        gt_poses=None, refine_depth_mm=None):
    """fit_mm: pose-fit tolerance in millimetres (None = off: the log is the plain pose log).  With it every log line also carries
    n_model and the inlier / front / behind shares of the model, and LOST? when the inlier share is under lost_below.  Track's record
    describes the pose the frame STARTED from (the previous frame's answer) against this frame's depth.
    render: beside every <id>_plot.png also write <id>_render.png, the overlay of fp_render_pose at the frame's pose (a silhouette shows
    a rotation about the object's long axis that the 12-edge box cannot).
    gt_poses: ground truth per frame (centred-mesh -> camera): also write errors.txt -- frame id, ADD, ADD-S, MSSD in metres, MSPD in
    pixels (fp_pose_errors, after the last frame: poses.txt and the plots do not change) -- and print the AUC of ADD and of ADD-S.
    refine_depth_mm: gate in millimetres (None = off): every Track answer is also refined on the frame's depth (fp_refine_depth, 10
    iterations) and refine.txt gets the frame id, the refined pose, n_used and rms_m; poses.txt and what Track starts from do not change."""
    seq = D.Sequence(data)
    mesh = load_mesh(name, seq.mesh_path())
    model = FoundationPose(mesh, seq.K, refiner, scorer, max_input_image_height=max(seq.H, 1080), max_input_image_width=max(seq.W, 1920))
    if fit_mm is not None:
        model.set_pose_fit(True, fit_mm * 1e-3)
    if depth_filter:
        model.set_depth_filter(True)
    os.makedirs(out, exist_ok=True)
    poses = []
    refined_log = open(os.path.join(out, "refine.txt"), "w") if refine_depth_mm is not None else None
    with open(os.path.join(out, "poses.txt"), "w") as log:
        def emit(i, pose, rgb, depth, plot, fit=None):
            tail = ""
            if fit is not None:
                tail = " fit %d %.4f %.4f %.4f" % (fit.n_model, fit.inlier_share, fit.front_share, fit.behind_share)
                if fit.inlier_share < lost_below:
                    tail += " LOST?"
                    print(f"{seq.ids[i]}: LOST? inliers {fit.inlier_share:.2f} front {fit.front_share:.2f} behind {fit.behind_share:.2f} of {fit.n_model} model pixels")
            log.write(seq.ids[i] + "".join(" %.9g" % v for v in to_colmajor(pose[None])[0]) + tail + "\n")
            if plot and render:
                model.upload_frame(rgb, depth)      # (a Track from a host frame uploaded only its crop window)
                over = model.render_pose(name, pose, want=("overlay",))["overlay"]
                _lib.lib().fp_image_write_png_rgb(os.path.join(out, seq.ids[i] + "_render.png").encode(), over.ctypes.data, seq.H, seq.W)
            if plot:
                img = D.draw_bbox3d(rgb, seq.K, D.convert_pose_mesh2bbox(pose, mesh), mesh.dimension)
                _lib.lib().fp_image_write_png_rgb(os.path.join(out, seq.ids[i] + "_plot.png").encode(), img.ctypes.data, seq.H, seq.W)
        rgb, depth, mask = seq.frame(0, with_mask=True)
        ok, pose = model.Register(rgb, depth, mask, name, refine_itr)
        if not ok:
            raise SystemExit(model.last_error)
        emit(0, pose, rgb, depth, True, model.last_register_fit() if fit_mm is not None else None)
        poses.append(pose)
        t0 = time.perf_counter()
        for i in range(1, len(seq)):
            rgb, depth = seq.frame(i)
            ok, pose = model.Track(rgb, depth, pose, name, refine_itr)
            if not ok:
                raise SystemExit(model.last_error)
            emit(i, pose, rgb, depth, plots or i + 1 == len(seq), model.last_track_fit()[0] if fit_mm is not None and refine_itr >= 1 else None)
            poses.append(pose)
            if refined_log is not None:
                model.upload_frame(rgb, depth)      # (a Track from a host frame uploaded only its crop window)
                better, (rec,) = model.refine_depth(name, pose, iterations=10, max_dist_m=refine_depth_mm * 1e-3)
                refined_log.write(seq.ids[i] + "".join(" %.9g" % v for v in to_colmajor(better)[0]) + " n_used %d rms_m %.9g\n" % (rec.n_used, rec.rms_m))
                print(f"{seq.ids[i]}: refined on the depth: n_used {rec.n_used}, rms {rec.rms_m * 1e3:.3f} mm after {rec.iterations} updates")
        if len(seq) > 1:
            print(f"tracked {len(seq) - 1} frames, {(len(seq) - 1) / (time.perf_counter() - t0):.1f} fps including PNG decode")
    if gt_poses is not None:
        errs = model.pose_errors(name, np.stack(poses), np.stack(gt_poses))
        with open(os.path.join(out, "errors.txt"), "w") as f:
            f.writelines("%s %.9g %.9g %.9g %.9g\n" % (fid, e.add_m, e.adds_m, e.mssd_m, e.mspd_px) for fid, e in zip(seq.ids, errs))
        print(f"ADD AUC {auc([e.add_m for e in errs]):.4f}, ADD-S AUC {auc([e.adds_m for e in errs]):.4f} (thresholds 0 .. 0.1 m) over {len(errs)} frames")
    if refined_log is not None:
        refined_log.close()
    model.close()
    return np.stack(poses)


def run_no_weights(data, out, name="mustard", plots=False, gt_poses=None, symmetries=None, gate_mm=20.0):
    """The sequence on a geometry-only model (no weights are read): the first frame's pose comes from fp_register_depth (the hypothesis grid
    ranked on the depth alone, the best candidates refined by ICP), every later frame's from fp_refine_depth started at the previous answer
    (15 iterations, gate gate_mm).  poses.txt gets the frame id, the pose, n_used and rms_m of the fit.
    gt_poses: ground truth per frame: every log line is followed on the console by the error against it, and errors.txt is written as by
    run().  symmetries: [S,4,4] of the mesh frame; with them MSSD / MSPD, the rotation and the translation are those against the nearest
    equivalent of the truth (the search cannot tell the equivalent poses of a symmetric object apart, and need not)."""
    seq = D.Sequence(data)
    mesh = load_mesh(name, seq.mesh_path())
    model = FoundationPose(mesh, seq.K, max_input_image_height=max(seq.H, 1080), max_input_image_width=max(seq.W, 1920))
    os.makedirs(out, exist_ok=True)
    poses = []
    with open(os.path.join(out, "poses.txt"), "w") as log:
        def emit(i, pose, rgb, rec, plot, how):
            log.write(seq.ids[i] + "".join(" %.9g" % v for v in to_colmajor(pose[None])[0]) + " n_used %d rms_m %.9g\n" % (rec.n_used, rec.rms_m))
            line = f"{seq.ids[i]}: {how}: n_used {rec.n_used}, behind {rec.n_behind}, rms {rec.rms_m * 1e3:.3f} mm after {rec.iterations} updates"
            if gt_poses is not None:
                e = model.pose_errors(name, pose[None], gt_poses[i], symmetries=symmetries, adds=False)[0]
                line += f"; against the truth: MSSD {e.mssd_m * 1e3:.3f} mm, {e.rot_deg:.3f} deg, {e.trans_m * 1e3:.3f} mm"
            print(line)
            if plot:
                img = D.draw_bbox3d(rgb, seq.K, D.convert_pose_mesh2bbox(pose, mesh), mesh.dimension)
                _lib.lib().fp_image_write_png_rgb(os.path.join(out, seq.ids[i] + "_plot.png").encode(), img.ctypes.data, seq.H, seq.W)
        rgb, depth, mask = seq.frame(0, with_mask=True)
        ok, pose, reg = model.register_depth(rgb, depth, mask, name)
        if not ok:
            raise SystemExit(model.last_error)
        emit(0, pose, rgb, reg.refine, True, f"registered on the depth (hypothesis {reg.hypothesis} of {reg.n_hypotheses}, {reg.n_candidates} refined, rank_key {reg.rank_key})")
        poses.append(pose)
        t0 = time.perf_counter()
        for i in range(1, len(seq)):
            rgb, depth = seq.frame(i)
            model.upload_frame(rgb, depth)
            refined, (rec,) = model.refine_depth(name, pose, iterations=15, max_dist_m=gate_mm * 1e-3)
            pose = refined[0]
            emit(i, pose, rgb, rec, plots or i + 1 == len(seq), "refined on the depth")
            poses.append(pose)
        if len(seq) > 1:
            print(f"followed {len(seq) - 1} frames, {(len(seq) - 1) / (time.perf_counter() - t0):.1f} fps including PNG decode")
    if gt_poses is not None:
        errs = model.pose_errors(name, np.stack(poses), np.stack(gt_poses), symmetries=symmetries)
        with open(os.path.join(out, "errors.txt"), "w") as f:
            f.writelines("%s %.9g %.9g %.9g %.9g\n" % (fid, e.add_m, e.adds_m, e.mssd_m, e.mspd_px) for fid, e in zip(seq.ids, errs))
        print(f"ADD-S AUC {auc([e.adds_m for e in errs]):.4f} (thresholds 0 .. 0.1 m), worst MSSD {max(e.mssd_m for e in errs) * 1e3:.3f} mm over {len(errs)} frames")
    model.close()
    return np.stack(poses)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data")
    ap.add_argument("--refiner")
    ap.add_argument("--scorer")
    ap.add_argument("--out", default="fp_demo_out")
    ap.add_argument("--name", default="mustard")
    ap.add_argument("--refine-itr", type=int, default=1)
    ap.add_argument("--plots", action="store_true")
    ap.add_argument("--fit", type=float, nargs="?", const=5.0, default=None, metavar="TOL_MM",
                    help="log the pose fit per frame (tolerance in mm, default 5) and mark frames whose inlier share is under --lost-below")
    ap.add_argument("--lost-below", type=float, default=0.5, metavar="SHARE")
    ap.add_argument("--depth-filter", action="store_true",
                    help="Register and Track read bilateral(erode(depth)) instead of the raw depth (FoundationPose as published); default off")
    ap.add_argument("--render", action="store_true",
                    help="beside every <id>_plot.png write <id>_render.png: the model at the frame's pose, its visible pixels flat-shaded over the frame; default off")
    ap.add_argument("--refine-depth", type=float, nargs="?", const=20.0, default=None, metavar="GATE_MM",
                    help="also refine every Track answer on the frame's depth (fp_refine_depth; gate in mm, default 20) and log n_used and rms_m to refine.txt; default off")
    ap.add_argument("--no-weights", action="store_true",
                    help="no networks: fp_register_depth on the first frame, then fp_refine_depth (15 iterations, gate 20 mm) per frame from the previous "
                         "answer; takes --data / --synthetic, --out, --name and --plots only; default off")
    ap.add_argument("--synthetic", type=int, metavar="N", help="write and use an N-frame synthetic sequence + synthetic weights")
    a = ap.parse_args()
    if a.no_weights:
        for flag, given in (("--refiner", a.refiner), ("--scorer", a.scorer), ("--fit", a.fit is not None), ("--depth-filter", a.depth_filter),
                            ("--render", a.render), ("--refine-depth", a.refine_depth is not None), ("--refine-itr", a.refine_itr != 1)):
            if given:
                ap.error(f"{flag} belongs to the modes that run the networks: --no-weights does not take it")
        gts = syms = None
        if a.synthetic:
            a.data = os.path.join(tempfile.mkdtemp(), "synthetic0")
            _, gts = D.write_synthetic_sequence(a.data, a.synthetic)
            syms = np.stack([np.diag(np.array(d, np.float32)) for d in ((1, -1, -1, 1), (-1, 1, -1, 1), (-1, -1, 1, 1))])   # the ellipsoid's
            print("synthetic sequence:", a.data, "(no weights: the poses are held to the scene's truth)")
        run_no_weights(a.data, a.out, a.name, a.plots, gts, syms)
        print("wrote", os.path.join(a.out, "poses.txt") + (" and errors.txt" if gts is not None else ""))
        return
    gts = None
    if a.synthetic:
        d = tempfile.mkdtemp()
        a.data = os.path.join(d, "synthetic0")
        _, gts = D.write_synthetic_sequence(a.data, a.synthetic)
        a.refiner, a.scorer = os.path.join(d, "refiner.fpw"), os.path.join(d, "scorer.fpw")
        W.pack_synthetic("refiner", a.refiner)
        W.pack_synthetic("scorer", a.scorer)
        print("synthetic sequence:", a.data, "(synthetic weights: poses are not meaningful, only reproducible)")
    run(a.data, a.refiner, a.scorer, a.out, a.name, a.refine_itr, a.plots, a.fit, a.lost_below, a.depth_filter, a.render, gts, a.refine_depth)
    print("wrote", os.path.join(a.out, "poses.txt") + (" and errors.txt" if gts is not None else ""))


if __name__ == "__main__":
    main()
