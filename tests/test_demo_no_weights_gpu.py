"""--no-weights of examples/demo_sequence.py: a geometry-only model registers the first frame of a synthetic sequence on the depth alone
and follows the others with fp_refine_depth; every frame ends at an equivalent of the scene's truth, and the weight-reading path of the
demo is not entered (no weight file exists)."""
import os
import sys

import numpy as np
import pytest

import search_cases as SC
from foundationpose_cpp_amd import dataset as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_weights_sequence_follows_the_truth(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import demo_sequence
    root = str(tmp_path / "synthetic0")
    _, gts = D.write_synthetic_sequence(root, 3)
    out = str(tmp_path / "out")
    poses = demo_sequence.run_no_weights(root, out, gt_poses=gts, symmetries=np.stack(SC.SYMMETRIES))
    text = capsys.readouterr().out
    print(text)
    assert poses.shape == (3, 4, 4)
    lines = open(os.path.join(out, "poses.txt")).read().splitlines()
    assert len(lines) == 3 and all(" n_used " in l and " rms_m " in l for l in lines)
    assert text.count("against the truth: MSSD") == 3 and "registered on the depth (hypothesis" in text
    errs = [[float(x) for x in l.split()[1:]] for l in open(os.path.join(out, "errors.txt")).read().splitlines()]
    # an equivalent of the truth: the bound of the device's Register on the 200 x 150 scenes (twice the float64 reference's worst MSSD,
    # search_cases.BOUND_M) plus the 1 mm to which the sequence's depth PNGs are quantised
    assert len(errs) == 3 and all(e[2] <= SC.BOUND_M + 0.001 for e in errs), errs
    assert os.path.exists(os.path.join(out, os.path.basename(sorted(os.listdir(os.path.join(root, "rgb")))[0]).replace(".png", "_plot.png")))
