"""The cases of tests/test_enc_tail_gpu.py: enc_tail_kernel, qkv_tile_kernel and enc_heads_kernel on caller-chosen operands through the test
build's raw hooks (fpt_enc_tail_raw, fpt_qkv_tile_raw, fpt_enc_heads_raw).  Pure Python + torch on the CPU: the class function, the input
families, the float64 reference (layer_ref.encoder_chain over explicit tensors), a plain float32 emulation of the kernel's arithmetic, the
comparators and the bounds.  tests/test_enc_tail_cases_cpu.py holds all of it to the library's plan and shows that the comparators can fail.

What selects code in enc_tail_kernel<DT, MI> (fp_nn_enc_kernels.inc):
  * MI in {1, 5} x DT in {f16, bf16}: the four instantiations (PF = 6 / 3 K-steps ahead, XD = 2 / 1 token-fragment buffers, KR = 1 / 3).
  * head: workgroups >= tiles read the second pointer set, so the heads of a problem never share a weight, bias or LayerNorm parameter.
  * tiles per head: the grid and the pdot offset of head 1; one tile, several, more than 256 workgroups' worth is not a code path.
  * token position in the tile: fragment mi (mi >= KR: x1 parked in lane-private LDS slots), li = token & 15, swizzle group li >> 2.
  * channel position (wave, g, k, e): channel 64 wave + 8 g + 32 k + e.  One-hot probe rows read every channel of every tile on its own.

Observability.  The kernel leaves pdot[head][tile][0..2] = sum_c S[c] * head_w[o][c], S = the column sums of the ROUNDED LayerNorm-2 output over
the tile's tokens, formed with fmaf in f32.  With a one-hot probe row every other product is +-0, so pdot is S[c] exactly; 171 probe sets
read all 512 columns (the hook launches the kernel once per set on the same operands); N_DENSE further sets are real read-out rows, held to
the dot product of the one-hot sums of the same call within the f32 accumulation error.

Error unit.  Nothing can be teacher-forced inside the kernel, so a flipped rounding of an intermediate propagates legitimately.  Per
LayerNorm-2 element the unit is one unit roundoff u of the LayerNorm-2 INPUT carried through the normalisation, plus the output's rounding:
    U = u * (|g| * rstd * (|y2| + mean_c |y2|) + |z|)          (all from the float64 reference)
and a column sum is held to K * sum_tokens U.  The K_* below are 2 x the peak of emulate() -- the same chain in float32 with f32 LayerNorm
statistics and the kernel's rounding points -- against the float64 chain over CASES (the factor: the emulation's summation order is not the
MFMA's; DESIGN.md section 2.1 uses the same convention for ETA).  test_enc_tail_cases_cpu.py re-measures them.

Where the LayerNorm stress sits.  A row whose mean is 300 times its spread in front of LayerNorm ONE would turn every flipped rounding of y1
(one in ~1000 elements between any two correct implementations) into 0.3 standard deviations of x1 -- hundreds of U, which no constant
could bound without blinding every other family.  The common mode is therefore built in front of LayerNorm TWO, whose input the unit
measures (gamma_1 = 0.1, beta_1 = 30), the constant and nearly constant rows in front of LayerNorm one (att = 0, b_o = 0: y1 = x without a
rounding; one exactly constant row per tile, make_problem says why), and the hundredfold channel in x.
"""
import zlib

import numpy as np
import torch

import layer_ref as LR

F16, BF16 = 0, 1
EMBED = 512
TOKENS = {1: 16, 5: 80}                                            # tokens per tile of enc_tail_kernel<., MI>
KR = {1: 1, 5: 3}                                                  # token fragments of x1 that stay in registers
LDS_TAIL = {1: 16 * 16 * 64 + 2 * 8 * 16 * 4, 5: 16 * 80 * 64 + 2 * 8 * 80 * 4 + 4 * 8192}
QKV_TOKENS, LDS_QKV = 80, 16 * 80 * 64
TAIL_ONE = {1: 1, 5: 2}                                            # fp_nn.hip TailForm of the instantiation
N_MAX = 2377
TORCH_DT = LR.TORCH_DT
DT_NAME = {F16: "f16", BF16: "bf16"}
DT_MAX = {F16: 65504.0, BF16: float(torch.finfo(torch.bfloat16).max)}
QNAN = {F16: 0x7E00, BF16: 0x7FC0}
N_ONEHOT, N_DENSE = 171, 2                                         # probe sets per hook call: 171 x 3 one-hot rows >= 512 columns, then dense rows
FAMILIES = ("iid", "live", "perm", "ln_mode", "ln_const", "ln_spike", "relu_dead", "relu_open")
# families under the statistical bound: every one but `live`, whose rows are compared one by one
INDEPENDENT = ("iid", "perm", "ln_mode", "ln_const", "ln_spike", "relu_dead", "relu_open")

# 2 x the emulation's peaks over CASES x EMULATIONS (test_enc_tail_cases_cpu.py::test_the_constants_are_twice_the_emulations_peaks re-measures):
#   per column sum or recovered element, any family 2.063 (live, MI = 5, f16);  16-token sums of independent tokens 0.2062;  80-token sums
#   0.05565;  |signed mean| of a case 1.05e-3 (i.i.d., MI = 1, f16, one tile: 1024 sums)
K_ELEM, K_16, K_80, K_MEAN = 4.2, 0.42, 0.115, 2.2e-3


def enc_class(MI, dt, tiles):
    """what selects code: the instantiation and whether the grid holds one tile per head or several (the head-1 offset is `tiles`)"""
    return ("enc_tail", MI, dt, min(tiles, 2))


def qkv_class(dt, tiles):
    """qkv_tile_kernel: the element type and how many of the three GEMM orders (blockIdx % 3) the grid holds"""
    return ("qkv_tile", dt, min(tiles, 3))


def _enc_cases():
    out = []
    for dt in (F16, BF16):
        for MI, counts in ((5, (1, 2, 7, 10)), (1, (1, 3, 25))):      # 7 / 3: odd counts; 25 at MI = 1: the workload's own shape (Track)
            out += [(MI, dt, t, "iid") for t in counts]
            out.append((MI, dt, TOKENS[MI] + 1, "live"))               # one live token per tile at every position + one all-zero tile
            out += [(MI, dt, 8 if fam in ("ln_mode", "ln_const") else (2 if MI == 5 else 3), fam) for fam in FAMILIES if fam not in ("iid", "live")]
    return out


CASES = _enc_cases()
QKV_CASES = [(dt, t, "iid") for dt in (F16, BF16) for t in (1, 2, 3, 7, 10)] + \
            [(dt, 3, fam) for dt in (F16, BF16) for fam in ("perm", "onehot")] + [(dt, 2, "top") for dt in (F16, BF16)]
HEADS_CASES = [(n, parts, fam, 0) for n in (1, 2, 3) for parts in (1, 5, 25) for fam in ("plain", "cancel", "huge")] + \
              [(1, parts, "plain", 1) for parts in (1, 5, 25)] + \
              [(n, parts, fam, 0) for n in (1, 3) for parts in (5, 25) for fam in ("rough_cancel", "rough_huge")]   # (n, parts, family, fused)


def case_id(c):
    MI, dt, tiles, fam = c
    return f"{fam}-MI{MI}-{DT_NAME[dt]}-t{tiles}"


def qkv_case_id(c):
    return f"{c[2]}-{DT_NAME[c[0]]}-t{c[1]}"


def heads_case_id(c):
    return f"{c[2]}-n{c[0]}-p{c[1]}{'-fused' if c[3] else ''}"


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def _to(a, dt):
    """numpy float64 -> torch tensor in the element type"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(TORCH_DT[dt])


def bits(t):
    """element-type tensor -> uint16 patterns"""
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(a, dt):
    return torch.from_numpy(a.view(np.int16).copy()).view(TORCH_DT[dt])


def _perm_matrix(rng):
    m = np.zeros((EMBED, EMBED))
    m[np.arange(EMBED), rng.permutation(EMBED)] = 1.0
    return m


class Problem:
    """operands of one enc_tail_kernel problem: att [2][rows][512] and x [rows][512] in the element type; W [2][3][512][512] (values of the
    element type, stored f32), b [2][3][512], g / be [2][2][512] f32; live [tiles] = the live token of a `live` tile (-1: the zero tile)"""


def make_problem(case):
    MI, dt, tiles, fam = case
    assert fam in FAMILIES
    rng, TOK = _rng("enc", *case), TOKENS[MI]
    rows = tiles * TOK
    n = lambda *s: rng.standard_normal(s)
    att, x = n(2, rows, EMBED), n(rows, EMBED)
    W = n(2, 3, EMBED, EMBED) / np.sqrt(EMBED)
    b = 0.3 * n(2, 3, EMBED)
    g, be = 1 + 0.1 * n(2, 2, EMBED), 0.3 * n(2, 2, EMBED)
    p = Problem()
    p.live = None
    if fam == "live":
        assert tiles == TOK + 1
        keep = np.zeros(rows, bool)
        p.live = np.append(np.arange(TOK), -1)
        keep[np.arange(TOK) * TOK + np.arange(TOK)] = True            # tile j: token j
        att[:, ~keep], x[~keep] = 0, 0
    elif fam == "perm":
        for h in range(2):
            for i in range(3):
                W[h, i] = _perm_matrix(rng)
    elif fam == "ln_mode":          # LayerNorm 2 sees a common mode of ~30 under a spread of ~0.1 (module docstring)
        g[:, 0], be[:, 0] = 0.1 * g[:, 0], 30 + 0.1 * be[:, 0]
        W[:, 1:] *= 0.05             # the FFN adds a few hundredths: y2 keeps x1's statistics
        b[:, 2] *= 0.1
    elif fam == "ln_const":         # in front of LayerNorm 1 (att = 0, b_o = 0: y1 = x) the odd tokens are constant up to +-2^-7 on a third of
        odd = np.arange(rows) % 2 == 1    # the channels each (variance 4e-5 against eps = 1e-5: the only rows on which eps is worth a tenth
        att[:, odd] = 0                   # of rstd), and ONE of them per tile, at another position in every tile, is exactly constant
        c = rng.choice([-1.0, 1.0], (rows, 1)) * rng.choice([1.0, 1.25, 1.5, 1.75], (rows, 1))     # (variance 0: rsqrt(eps) applies).
        near = rng.integers(-1, 2, (rows, EMBED)) * 2.0 ** -7                 # One per tile, because LayerNorm 1 turns EVERY constant row into
        p.const_rows = np.arange(tiles) * TOK + (22 * np.arange(tiles) + 1) % TOK      # beta_1: k of them in a tile are one token k times, whose
        near[p.const_rows] = 0                                                # every flipped rounding costs a column sum k ulps at once --
        x[odd] = (c + near)[odd]                                              # with 20 of 80, a median 0.106 of sum U against K_80 = 0.115
        b[:, 0] = 0
    elif fam == "ln_spike":         # one channel a hundred times the rest, another one per token fragment
        ch = (np.arange(rows) // 16 * 37 + 5) % EMBED
        x[np.arange(rows), ch] *= 100
    elif fam == "relu_dead":        # b1 so negative that the hidden layer is all zero: y2 = b2 + x1
        b[:, 1] = -1000 + b[:, 1]
    elif fam == "relu_open":        # b1 so positive that nothing is clipped
        b[:, 1] = 50 + b[:, 1]
    p.MI, p.dt, p.tiles, p.fam, p.TOK, p.rows = MI, dt, tiles, fam, TOK, rows
    p.att, p.x = _to(att, dt), _to(x, dt)
    p.W = _to(W, dt).float()
    p.b, p.g, p.be = (torch.from_numpy(a).float() for a in (b, g, be))
    return p


def probes(case):
    """head_w [P][2][3][512] f32: N_ONEHOT one-hot sets (set p, row o: column 3 p + o, a zero row past column 511; both heads alike), then
    N_DENSE sets of real read-out rows, another draw per head"""
    w = np.zeros((N_ONEHOT + N_DENSE, 2, 3, EMBED), np.float32)
    for c in range(EMBED):
        w[c // 3, :, c % 3, c] = 1.0
    w[N_ONEHOT:] = 0.05 * _rng("probe", *case).standard_normal((N_DENSE, 2, 3, EMBED))
    return w


# ---- the chain: float64 reference, float32 emulation, and every mutation of the negative controls -------------------------------------------
NAMES = {k: k for k in ("out_w", "out_b", "l1_w", "l1_b", "l2_w", "l2_b", "ln1", "ln2")}       # tensor names of reference_chain's dictionary


def reference_chain(p, h):
    """layer_ref.encoder_chain on the problem's tensors: float64, y1, x1, hid, y2 rounded; ln2 unrounded"""
    t = {"out_w": p.W[h, 0], "out_b": p.b[h, 0], "l1_w": p.W[h, 1], "l1_b": p.b[h, 1], "l2_w": p.W[h, 2], "l2_b": p.b[h, 2],
         "ln1.weight": p.g[h, 0], "ln1.bias": p.be[h, 0], "ln2.weight": p.g[h, 1], "ln2.bias": p.be[h, 1]}
    return LR.encoder_chain(LR.TensorWeights(t, p.dt), h, p.x, p.att[h], names=NAMES, readout=False)


def trunc(t, dt):
    """t rounded TOWARD ZERO to the element type (the controls' wrong rounding)"""
    r = t.to(TORCH_DT[dt])
    over = r.to(t.dtype).abs() > t.abs()
    return torch.where(over, r.view(torch.int16) - 1, r.view(torch.int16)).view(TORCH_DT[dt]).to(t.dtype)


EMULATIONS = ("plain", "kstep", "kstep_exact")     # summation orders of the float32 emulation (chain, mm)


def chain(p, h, f32=False, wh=None, order="plain", **mut):
    """The same chain written out: float64 (no mutation: equal to reference_chain, the CPU test holds it to that) or, f32 = True, the
    kernel's arithmetic -- f32 products and sums, (acc + bias) + residual, two-pass f32 LayerNorm statistics, the same five roundings.
    order: how the f32 emulation adds up a GEMM (EMULATIONS): nobody outside the matrix unit knows its order, so the constants take the peak
    over three plausible ones -- which also triples the draws of rounding noise that the signed-mean constant is twice the peak of.
    wh: the head whose parameters are used (control: head 1 with head 0's weights).  mut: the negative controls
      drop=(gemm, fragment, kstep)  no_res1, no_res3, res3_unrounded, no_relu, eps=, swap_ln, bias_shift=(which, c0), trunc=stage, x_shift=rows
    -> dict y1, x1, hid, y2, ln2 (unrounded), z (rounded)"""
    T = torch.float32 if f32 else torch.float64
    dt, wh = p.dt, h if wh is None else wh
    stage = mut.get("trunc")
    rn = lambda t, name: (trunc(t, dt) if stage == name else t.to(TORCH_DT[dt]).to(T))
    W = [p.W[wh, i].to(TORCH_DT[dt]).to(T) for i in range(3)]
    b = [p.b[wh, i].to(T).clone() for i in range(3)]
    if "bias_shift" in mut:
        i, c0 = mut["bias_shift"]
        b[i][c0:c0 + 8] = p.b[wh, i].to(T)[c0 + 8:c0 + 16]
    ln = [(p.g[wh, i].to(T), p.be[wh, i].to(T)) for i in range(2)]
    if mut.get("swap_ln"):
        ln = ln[::-1]
    eps = mut.get("eps", 1e-5)
    att, x = p.att[h].to(T), p.x.to(T)
    if "x_shift" in mut:
        x = torch.roll(x, -mut["x_shift"], 0)

    def mm(a, w, q):
        if order == "plain":
            y = a @ w.T
        else:          # 32-channel K-steps added up in f32 in the kernel's order; "kstep_exact": each step's 32 products summed exactly first
            y = torch.zeros(a.shape[0], w.shape[0], dtype=T)
            for s in range(0, EMBED, 32):
                y = y + ((a[:, s:s + 32].double() @ w[:, s:s + 32].double().T).to(T) if order == "kstep_exact" else a[:, s:s + 32] @ w[:, s:s + 32].T)
        if mut.get("drop", (None,))[0] == q:
            _, frag, ks = mut["drop"]
            t, k = slice(16 * frag, 16 * frag + 16), slice(32 * ks, 32 * ks + 32)
            y[t] = y[t] - a[t, k] @ w[:, k].T
        return y

    def norm(y, gb):
        mu = y.mean(-1, keepdim=True)
        var = ((y - mu) ** 2).mean(-1, keepdim=True)
        return (y - mu) * (1.0 / torch.sqrt(var + eps)) * gb[0] + gb[1]

    r = {}
    y = mm(att, W[0], 0) + b[0]
    r["y1"] = rn(y if mut.get("no_res1") else y + x, "y1")
    x1u = norm(r["y1"], ln[0])
    r["x1"] = rn(x1u, "x1")
    y = mm(r["x1"], W[1], 1) + b[1]
    r["hid"] = rn(y if mut.get("no_relu") else y.clamp_min(0.0), "hid")
    y = mm(r["hid"], W[2], 2) + b[2]
    r["y2"] = rn(y if mut.get("no_res3") else y + (x1u if mut.get("res3_unrounded") else r["x1"]), "y2")
    r["ln2"] = norm(r["y2"], ln[1])
    r["z"] = rn(r["ln2"], "z")
    return r


def column_sums(z, p, f32=False):
    """[rows][512] -> [tiles][512]: the tile's column sums (f32 = True: summed in float32 like the kernel's)"""
    return (z.float() if f32 else z).reshape(p.tiles, p.TOK, EMBED).sum(1).double()


def reference(p):
    """-> dict z [2][rows][512] (rounded LayerNorm-2 output), U (the error unit per element), S, SU [2][tiles][512] (column sums of both),
    peak (the largest |intermediate| of the chain, asserted below half the element type's maximum)"""
    u = LR.UNIT[p.dt]
    zs, Us, peak = [], [], 0.0
    for h in range(2):
        r = reference_chain(p, h)
        y2, g = r["y2"], p.g[h, 1].double()
        rstd = 1.0 / torch.sqrt(((y2 - y2.mean(-1, keepdim=True)) ** 2).mean(-1, keepdim=True) + 1e-5)
        z = LR.rnd(r["ln2"], p.dt)
        zs.append(z)
        Us.append(u * (g.abs() * rstd * (y2.abs() + y2.abs().mean(-1, keepdim=True)) + z.abs()))
        peak = max(peak, max(float(r[k].abs().max()) for k in ("y1", "x1", "hid", "y2", "ln2")))
    assert peak <= 0.5 * DT_MAX[p.dt], peak
    z, U = torch.stack(zs), torch.stack(Us)
    return {"z": z, "U": U, "peak": peak, "S": torch.stack([column_sums(z[h], p) for h in range(2)]),
            "SU": torch.stack([column_sums(U[h], p) for h in range(2)])}


def emulate(p, order="plain"):
    """-> S [2][tiles][512] as float64: the column sums the plain float32 emulation of the kernel leaves"""
    return torch.stack([column_sums(chain(p, h, f32=True, order=order)["z"], p, f32=True) for h in range(2)])


def mutated_sums(p, **mut):
    """-> S [2][tiles][512] of the float64 chain under a control's mutation (head_swap: head 1 with head 0's parameters)"""
    swap = mut.pop("head_swap", False)
    return torch.stack([column_sums(chain(p, h, wh=0 if swap else h, **mut)["z"], p) for h in range(2)])


# ---- comparators -------------------------------------------------------------------------------------------------------------------------
def _ratio(err, unit):
    return torch.where(unit > 0, err / unit.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))


def compare(p, ref, S):
    """column sums S [2][tiles][512] (float64 values of what the device or an emulation left) against the reference
    -> dict worst (max |dS| / sum U over every column sum; `live`: over every recovered element), mean (the signed mean of
    sign(ref) * d / U over the same set), n (its size)"""
    if p.fam != "live":
        d, unit, sign = S - ref["S"], ref["SU"], torch.sign(ref["S"])
    else:        # tile j holds ONE live token at position j and TOK - 1 zero rows, the last tile TOK zero rows: the live row of z is
                 # S_tile - (TOK - 1) / TOK * S_zero_tile (every zero row of a head leaves the same z, on the device as in the reference)
        TOK = p.TOK
        got = S[:, :TOK] - (TOK - 1) / TOK * S[:, TOK:]
        idx = torch.arange(TOK) * TOK + torch.arange(TOK)
        zl = ref["z"][:, idx]
        d, unit, sign = got - zl, ref["U"][:, idx], torch.sign(zl)
    r = _ratio(d.abs(), unit)
    return {"worst": float(r.max()), "mean": float((sign * d / unit.clamp_min(1e-300)).mean()), "n": d.numel()}


def limits(p):
    """(hard bound, statistical bound or None, signed-mean bound) of a case in units of sum U"""
    stat = None if p.fam not in INDEPENDENT else (K_16 if p.TOK == 16 else K_80)
    return K_ELEM, stat, K_MEAN


def verdict(p, c):
    """the assertions of a comparison as a list of the names of those that FAIL: 'hard', 'stat', 'mean'"""
    hard, stat, mean = limits(p)
    out = []
    if not c["worst"] <= hard:
        out.append("hard")
    if stat is not None and not c["worst"] <= stat:
        out.append("stat")
    if not abs(c["mean"]) <= mean:
        out.append("mean")
    return out


def emulation_peaks(cases=None):
    """every emulation order over the case list against the float64 chain -> ({"elem", "k16", "k80", "mean"}: the peaks the constants are
    twice of, rows: (case, order, comparison) of every run)"""
    peaks, rows = {"elem": 0.0, "k16": 0.0, "k80": 0.0, "mean": 0.0}, []
    for case in cases or CASES:
        p = make_problem(case)
        ref = reference(p)
        for order in EMULATIONS:
            c = compare(p, ref, emulate(p, order))
            rows.append((case, order, c))
            peaks["elem"] = max(peaks["elem"], c["worst"])
            if p.fam in INDEPENDENT:
                k = "k16" if p.TOK == 16 else "k80"
                peaks[k] = max(peaks[k], c["worst"])
            peaks["mean"] = max(peaks["mean"], abs(c["mean"]))
    return peaks, rows


def dense_reference(S, hw):
    """the DENSE probe sets against the column sums S [2][tiles][512] the SAME call returned through its one-hot sets: hw [D][2][3][512] ->
    (pdot [D][2][tiles][3] in float64, bound): the two paths differ by the f32 accumulation of the fmaf chain alone, C_ACC * sum_c |S_c w_c|
    (layer_ref: the f32 accumulation figure up to K = 1024)"""
    w = torch.from_numpy(hw).double()
    return torch.einsum("htc,dhoc->dhto", S, w), LR.C_ACC * torch.einsum("htc,dhoc->dhto", S.abs(), w.abs())


def sums_from_pdot(pdot):
    """pdot [P][2][tiles][4] of a hook call -> S [2][tiles][512]: column c = slot c % 3 of one-hot set c // 3"""
    c = np.arange(EMBED)
    return torch.from_numpy(pdot[c // 3, :, :, c % 3].astype(np.float64)).permute(1, 2, 0).contiguous()


# ---- qkv_tile_kernel ---------------------------------------------------------------------------------------------------------------------
def make_qkv_problem(case):
    """-> (x [80 tiles][512] element type, W [1536][512] f32 holding element-type values, bias [1536] f32, exact): exact = the output must
    equal the rounded float64 reference bit for bit (every sum is one product that f32 holds exactly, the bias on the element type's grid)"""
    dt, tiles, fam = case
    rng = _rng("qkv", *case)
    rows = tiles * QKV_TOKENS
    x = rng.standard_normal((rows, EMBED))
    W = rng.standard_normal((3 * EMBED, EMBED)) / np.sqrt(EMBED)
    b = 0.3 * rng.standard_normal(3 * EMBED)
    if fam in ("perm", "top"):       # every output = +-x[one channel] + bias, another channel order in each of Q, K, V
        W = np.concatenate([_perm_matrix(rng) for _ in range(3)]) * rng.choice([-1.0, 1.0], (3 * EMBED, 1))
        b = np.round(4 * b) / 4                                    # multiples of 1/4 below 2: x + b needs no more bits than f32 has
        x = np.round(64 * x) / 64
    if fam == "top":                 # values in the upper half of the range; a bias of +-2^-7 of the top binade carries the largest of them over
        top = DT_MAX[dt]             # the threshold where the reference rounds to infinity, as the device's conversion does
        x = rng.choice([-1.0, 1.0], x.shape) * top * (1 - rng.integers(0, 256, x.shape) / 512)
        b = rng.choice([-1.0, 0.0, 1.0], b.shape) * 2.0 ** (np.floor(np.log2(top)) - 7)
    if fam == "onehot":              # one channel per token is non-zero: a single product per output, no bias
        keep = np.zeros_like(x, bool)
        keep[np.arange(rows), (np.arange(rows) * 29 + 3) % EMBED] = True
        x, b = np.where(keep, 1 + np.abs(x), 0.0), 0 * b
    return _to(x, dt), _to(W, dt).float(), torch.from_numpy(b).float(), fam != "iid"


def qkv_reference(x, W, b):
    """-> (unrounded float64 [rows][1536], acc)"""
    x, W, b = x.double(), W.double(), b.double()
    return x @ W.T + b, LR.C_ACC * (x.abs() @ W.abs().T + b.abs())


def qkv_emulate(x, W, b):
    return (x.float() @ W.float().T + b).to(x.dtype)


# ---- enc_heads_kernel --------------------------------------------------------------------------------------------------------------------
SEQ_TOKENS = 400.0


def make_heads_problem(case):
    """-> (pdot [2][n * parts][4] f32 with NaN in slot 3 -- the kernel must not read it --, bias [2][3] f32).  Every share is a multiple of
    1/8 below 2^20, so every partial sum is exact in f32 in any order: two roundings remain (the division, the bias), half an ulp each,
    which is what a bound of ONE ulp can hold for every correct implementation; a sum that loses bits (a huge tile swallowing the others,
    cancelling tiles leaving their rounding) does not get that far.  The rough_* families are the same stress OFF the grid, where every
    add rounds, under the bound that grows with `parts` (heads_reference)."""
    n, parts, fam, _ = case
    rng = _rng("heads", *case)
    pd = np.round(800 * rng.standard_normal((2, n, parts, 4))) / 8
    if fam == "cancel" and parts > 1:        # tiles that cancel to 1/8 each
        pd[:, :, 1::2] = -(pd[:, :, 0:2 * (parts // 2):2] + 0.125)
    elif fam == "huge":                      # one tile ~5000 times the others
        pd[:, :, parts // 2] = rng.choice([-1.0, 1.0], (2, n, 4)) * rng.choice([1.0, 1.5], (2, n, 4)) * 2.0 ** 19
    elif fam.startswith("rough"):            # the same stress OFF the grid: every add rounds (bound: heads_reference)
        pd = 100 * rng.standard_normal((2, n, parts, 4))
        if fam == "rough_cancel":
            pd[:, :, 1::2] = -pd[:, :, 0:2 * (parts // 2):2] * (1 + 1e-4)
        else:
            pd[:, :, parts // 2] *= 1e6
    pd = pd.astype(np.float32)
    pd[..., 3] = np.nan
    return pd.reshape(2, n * parts, 4), (0.3 * rng.standard_normal((2, 3))).astype(np.float32)


def heads_reference(pd, bias, n, parts, rough=False):
    """-> (y [2][n][3] float64, bound: one f32 ulp of sum |parts| / tokens + |bias|, y32: the sequential float32 emulation).
    rough (shares off the grid): `parts` ulps -- each of the parts - 1 adds rounds a partial sum of at most sum |parts| by half an ulp
    of it, which after the division is less than one ulp of sum |parts| / tokens; the division and the bias share the last one"""
    v = pd.reshape(2, n, parts, 4)[..., :3].astype(np.float64)
    y = v.sum(2) / SEQ_TOKENS + bias[:, None, :]
    mag = np.abs(v).sum(2) / SEQ_TOKENS + np.abs(bias[:, None, :].astype(np.float64))
    bound = np.spacing(mag.astype(np.float32)).astype(np.float64) * (parts if rough else 1)
    s = pd.reshape(2, n, parts, 4)[:, :, 0, :3].copy()
    for t in range(1, parts):
        s = s + pd.reshape(2, n, parts, 4)[:, :, t, :3]
    y32 = s / np.float32(SEQ_TOKENS) + bias[:, None, :]
    return y, bound, y32.astype(np.float32)
