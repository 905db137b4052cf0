"""The device's render + crop stage against the float64 references of tests/shade_warp_ref.py: the three comparisons of
tests/test_shade_warp_ref_cpu.py with the outputs of `FoundationPose.debug_rasterize` / `render_and_transform` in the oracle's place.

Cases, bounds, exemptions and caps are that module's, imported; nothing is tuned here.  shade_ref is fed the DEVICE's own rasteriser
output, both float models run (the references do not depend on the model, the bounds cover both), and `rast[..., 3]` has to equal the
triangle-id buffer, which tests/test_geometry_gpu.py holds bit-exact to the oracle.  The module prints one table: per case the peaks as
fractions of their bounds and the exempted shares."""
import numpy as np
import pytest

import test_shade_warp_ref_cpu as C
from foundationpose_cpp_amd import FoundationPose

pytestmark = pytest.mark.gpu

_TABLE = []


@pytest.fixture(scope="module", autouse=True)
def table():
    yield
    print("\n  device against the float64 references (peaks as fractions of their bounds; eta, eta_w as fractions of ETA, ETA_W):")
    for row in _TABLE:
        C.print_row(*row)


def _device_outputs(m, c, ratio):
    tri, rast = m.debug_rasterize(c.mesh.name, c.poses, ratio)
    render, _ = m.render_and_transform(c.mesh.name, c.poses, ratio)
    _, crop = m.render_and_transform(c.mesh.name, C.warp_poses(c.name, ratio), ratio)
    return tri, rast, render, crop


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_device_matches_the_float64_references(name):
    c = C.case(name)
    m = FoundationPose(c.mesh, c.K)
    failures = []
    try:
        m.upload_frame(c.rgb, c.depth)
        for fmad in (1, 0):
            m.set_float_model(fmad)
            for ratio in c.ratios:
                tri, rast, render, crop = _device_outputs(m, c, ratio)
                for kind, check in (("shade", lambda: C.check_case_shade(c, render, rast)),
                                    ("bary", lambda: C.check_case_bary(c, ratio, rast, tri)),
                                    ("warp", lambda: C.check_case_warp(c, ratio, crop))):
                    try:
                        s = check()
                        _TABLE.append((kind, name, ratio, s, f"fmad={fmad}"))
                        if kind == "shade":
                            assert s["colour"] < C.HALF and s["xyz"] < C.HALF, f"a peak above half of its bound: {s}"
                    except AssertionError as e:
                        failures.append(f"{kind} ratio {ratio} fmad={fmad}: {e}")
    finally:
        m.close()
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", ["rnd1", "wquad"])
def test_wrong_rules_fail_on_the_device_outputs_too(name):
    """the comparisons keep their teeth with the device's outputs in place of the oracle's: every wrong texture rule fails the colour bound,
    a sample point without the half pixel fails the barycentric bound"""
    c = C.case(name)
    m = FoundationPose(c.mesh, c.K)
    try:
        m.upload_frame(c.rgb, c.depth)
        tri, rast, render, _ = _device_outputs(m, c, 1.2)
    finally:
        m.close()
    assert (tri > 0).any()
    for rule, sampler in C.WRONG_SAMPLERS.items():
        with pytest.raises(AssertionError, match="colour off"):
            C.check_case_shade(c, render, rast, sampler)
    with pytest.raises(AssertionError, match="values off"):
        C.check_case_bary(c, 1.2, rast, offset=(0.0, 0.0))

