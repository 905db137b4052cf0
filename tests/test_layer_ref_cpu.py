"""The float64 stage reference (tests/layer_ref.py) chained over a whole network IS the network of oracle/nets_torch.py.

With element-type rounding off, the stages chained from a host-built nn_in must give the refiner's trans / rot and the scorer's scores
of the torch oracle run in float64, to 1e-5 of the output scale -- the only expected difference being that the folded weights of the
.fpw are stored in f32.  This pins the reference that tests/test_layers_gpu.py compares every device stage with."""
import numpy as np
import pytest
import torch

from foundationpose_cpp_amd import weights as W
from oracle import nets_torch as NT
import layer_ref as LR
from nn_in_ref import nn_in_from_blobs      # the layout of the device's network input (tests/test_nn_in_ref_cpu.py holds it to the address formula)


@pytest.fixture(scope="module")
def blobs():
    rng = np.random.default_rng(3)
    N = 2
    return rng.uniform(-1, 1, (N, 160, 160, 6)).astype(np.float32), rng.uniform(-1, 1, (N, 160, 160, 6)).astype(np.float32)


def _torch64(kind, state):
    return NT.build(kind, state).double()


def test_nn_in_layout_matches_the_stem_input(blobs):
    a, b = blobs
    x = nn_in_from_blobs(a, b)
    assert x.shape == (4, 84, 84, 32)
    assert float(x[:, :2].abs().sum() + x[:, -2:].abs().sum()) == 0.0
    assert x[0, 2 + 7, 2 + 11, (1 * 2 + 0) * 8 + 4] == np.float64(a[0, 15, 22, 4])   # pixel (2*7+1, 2*11+0), channel 4


@pytest.mark.parametrize("seed", [9])
def test_refiner_chain_equals_oracle_float64(tmp_path, blobs, seed):
    path = str(tmp_path / "r.fpw")
    st = W.pack_synthetic("refiner", path, seed)
    w = LR.Weights(path, None)
    a, b = blobs
    N = len(a)
    pe = torch.from_numpy(LR.pos_table()).double()
    acts = LR.trunk_chain(w, nn_in_from_blobs(a, b), N, N, pe)
    x = acts[-1]
    outs = []
    for h in range(2):
        n = LR.refiner_head_names(h)
        qkv, _ = LR.linear(w, n["in_w"], n["in_b"], x)
        att, _ = LR.sdpa(qkv, None)
        outs.append(LR.encoder_chain(w, h, x, att)["out"])
    with torch.no_grad():
        rt, rr = _torch64("refiner", st)(torch.from_numpy(a).double(), torch.from_numpy(b).double())
    for got, ref in zip(outs, (rt, rr)):
        scale = float(ref.abs().max())
        assert scale > 0
        err = float((got - ref).abs().max())
        assert err <= 1e-5 * scale, (err, scale)


def test_scorer_chain_equals_oracle_float64(tmp_path, blobs):
    path = str(tmp_path / "s.fpw")
    st = W.pack_synthetic("scorer", path, 9)
    w = LR.Weights(path, None)
    a, b = blobs
    N = len(a)
    pe = torch.from_numpy(LR.pos_table()).double()
    x = LR.trunk_chain(w, nn_in_from_blobs(a, b), N, N, pe)[-1]
    qkv, _ = LR.linear(w, "att.in_proj_weight", "att.in_proj_bias", x)
    att, _ = LR.sdpa(qkv, None)
    feat, _ = LR.linear(w, "att.out_proj.weight", "att.out_proj.bias", att.mean(1), out_dt=None, f32_weights=True)
    xq, _ = LR.linear(w, "att_cross.in_proj_weight", "att_cross.in_proj_bias", feat)
    xa, _ = LR.sdpa(xq[None], None)
    xo, _ = LR.linear(w, "att_cross.out_proj.weight", "att_cross.out_proj.bias", xa[0])
    scores, _ = LR.linear(w, "linear.weight", "linear.bias", xo, out_dt=None, f32_weights=True)
    with torch.no_grad():
        net = _torch64("scorer", st)
        ref_feat = net.extract_feat(torch.from_numpy(a).double(), torch.from_numpy(b).double())
        ref = net.head(ref_feat)
    assert float((feat - ref_feat).abs().max()) <= 1e-5 * float(ref_feat.abs().max())
    scale = float(ref.abs().max())
    assert float((scores.reshape(-1) - ref).abs().max()) <= 1e-5 * scale, (scores, ref)


def test_rounding_helpers():
    t = torch.tensor([1.0, 1.0 + 2 ** -11, 1.0 + 3 * 2 ** -11, 3e-8, 65504.0], dtype=torch.float64)
    r = LR.rnd(t, LR.F16)
    assert r.tolist() == [1.0, 1.0, 1.0 + 4 * 2 ** -11, 2 ** -24, 65504.0]     # ties to even
    assert LR.ulp(torch.tensor([1.0, 0.75, 0.0], dtype=torch.float64), LR.F16).tolist() == [2 ** -10, 2 ** -11, 2 ** -24]
    assert LR.ulp(torch.tensor([1.0], dtype=torch.float64), LR.BF16).tolist() == [2 ** -7]
