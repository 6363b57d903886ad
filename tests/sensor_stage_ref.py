"""TEST INFRASTRUCTURE ONLY -- the sensor stage (observation embedding, both Observation_progation layers, the [F, T d] -> [T, F d]
scatter, the PE columns and the padding mask behind rd_sensor_stage_fwd / rd_msgpass_bwd): case table, inputs and float64 reference.

Used by tests/test_sensor_stage_ref_host.py (conditions on the reference alone, no GPU) and tests/test_sensor_stage_float64_gpu.py
(the fused kernels of rd_msgpass_fused.hip / rd_msgpass_dw.hip across their envelope, the generic path just outside it and in fp32
mode, the padded layout and a registered token plan, against this reference).

Reference (plain numpy float64, batched; nothing comes from the device except the coefficient table of the COEF cases, which is DATA):
    X [b, f, 4t+c] = relu(src[t, b, f] * R_u[4f+c])
    Y1 = relu(X W1^T + b1) * s1[b, f]          Y2 = relu(Y1 W2^T + b2) * s2[b, f]          z[t, b, 4f+c] = Y2[b, f, 4t+c]
    s1 = s2 = ssum[f], or rows 0 / 1 of a coefficient table [2, B, F] (COEF cases)
and, for a given dz, the gradients of R_u, W1, b1, W2, b2 by the chain rule written out (tests/test_sensor_stage_ref_host.py holds
them to torch autograd on oracle/restatement.py observation_propagation and to a central finite difference).  On a token plan the
reference zeroes dz at steps t >= length and z / PE are compared on live rows only (`to_plan`); on the padded layout all T steps are
live.  Observations are zero at steps >= a sample's length in every case (no plan slack: the step-level tests own that path).
PE: the fp32 angle times / timescale of oracle/restatement.py positional_encoding, its sine and cosine taken in float64.

Scale of the inputs: observed values N(0, 1) at density 0.5, R_u = 1.5 N(0, 1) / sqrt(share of live steps) (so that samples of one
step still give pre-activations of standard deviation 0.5 .. 1), W1, W2 = N(0, 1 / K), ssum = U(0.5, 1.5) per sensor (distinct per
sensor, so exchanging two of them shows; the stage takes ssum as an argument), dz = N(0, 1).  max |z| then lies in [1/8, 8] -- O(1) --
in all but a few cases and z is compared in absolute terms there; where it does not (one-step samples: up to 15; F = 1 with five
rows: down to 0.05) the error is divided by max |z_ref| (z_scale).

Decisive, row-dependent gates.  b1[n] = -(midpoint of the widest gap between consecutive distinct values, inside the 25 % .. 75 % rank
range, of column n of X W1^T over all B F graph rows and the value 0.0 of an all-zero row), rounded to fp32; then b2[n] the same way
from Y1 W2^T.  About half of every column's rows are open, WHICH rows differs per column and per row, and every pre-activation of
both layers keeps |pre| >= GATE_MARGIN = 1e-3 (absolute; a condition every case meets in the reference alone -- a case that misses it
gets another seed, SEED_BUMP, never another margin).  Every non-zero src * R_u is a normal fp32 number, so the X gate is exact too.
With no gate able to flip, no entry is exempt and no share of entries may miss.

Bounds (bound_of): z 2e-5 x 6 absolute in bf16x3 and 2e-5 in fp32 (test_sensor_stage_vs_oracle); PE 2e-6; the mask bit-exact; every
gradient 2e-4 of its float64 max-norm (test_attention_core_vs_float64, plan_layer_ref.GRAD_REL), raised per tensor to 2 x the
YARDSTICK's measured error where that exceeds 1e-4.  The yardstick is the same padded-layout cases under RD_K1_FUSED=0 -- the generic
kernels test_sensor_stage_vs_oracle binds.  No bound is taken from the fused path."""
import functools
import zlib

import numpy as np
import torch

from oracle import restatement as O2
from tests.helpers import plan_ref

D_OB, D_PE = 4, 16
GATE_MARGIN = 1e-3
MAX_ROWS = 1600
GRAD_NAMES = ("R_u", "W1", "b1", "W2", "b2")
MODES = ("bf16x3", "fp32")
COEF_P, COEF_SEED = (0.3, 0.3), 77

# ---- shapes: name -> (F, T, B, observation pattern) -----------------------------------------------------------------------------------
# Row-tile grouping of rd_k1_layout.h: q = F / 32 main tiles per sample, rem = F % 32 leftover rows, per = 32 / rem samples per
# leftover tile.  RT = ceil(F / 16) selects the instantiation; nct = T / 4 column tiles; the reduction runs ceil(K / 32) steps.
SHAPES = {
    # leftover-tile geometry, B around `per`
    "F1_B3": (1, 4, 3, "dense"),          # per 32: one leftover tile, 3 of 32 positions covered, S = 1 < 4, nct = 1, K < 32
    "F1_B33": (1, 8, 33, "dense"),        # per 32: a full tile and a second one with a single sample
    "F5": (5, 12, 7, "dense"),            # per 6: positions 30, 31 belong to no sample; second tile holds one sample
    "F16": (16, 20, 3, "dense"),          # per 2, rem 16: no uncovered position in a full tile; B odd
    "F17": (17, 32, 3, "dense"),          # per 1: 15 uncovered positions in every tile, RT = 2
    "F31": (31, 48, 2, "dense"),          # per 1: one uncovered position
    "F32": (32, 56, 3, "dense"),          # rem 0: no leftover tile at all, S = 3 < 4
    "F33": (33, 60, 5, "dense"),          # q 1 + rem 1, per 32, RT = 3 at run-time T = 60
    "F34_B15": (34, 60, 15, "dense"),     # per 16: one short of a full leftover tile (the specialised instantiation)
    "F34_B16": (34, 60, 16, "dense"),     # exactly full
    "F34_B17": (34, 60, 17, "dense"),     # one over
    "F34_T56": (34, 56, 9, "dense"),      # the runtime-shape RT = 3 instantiation by default, K % 32 == 0
    "F47": (47, 20, 3, "dense"),          # rem 15, per 2: positions 30, 31 uncovered
    "F48": (48, 12, 3, "dense"),          # rem 16, per 2, the envelope's last F
    # one sample, one F per row-tile count
    "B1_RT1": (16, 32, 1, "dense"), "B1_RT2": (32, 8, 1, "dense"), "B1_RT3": (48, 48, 1, "dense"),
    # `lin` patterns mixed in one batch (see _observed)
    "LIN_P19": (34, 60, 8, "lin"), "LIN_RT1": (16, 32, 6, "lin"),
    # just outside the envelope: the routing edge (generic path in both modes)
    "F49": (49, 60, 3, "dense"), "T61": (34, 61, 3, "dense"), "T15": (34, 15, 3, "dense"),
    # COEF instantiations, one per RT and the specialised one
    "C_RT1": (16, 32, 5, "dense"), "C_RT2": (32, 20, 3, "dense"), "C_RT3": (34, 56, 5, "dense"), "C_P19": (34, 60, 5, "dense"),
}
GEOMETRY = ("F1_B3", "F1_B33", "F5", "F16", "F17", "F31", "F32", "F33", "F34_B15", "F34_B16", "F34_B17", "F34_T56", "F47", "F48",
            "B1_RT1", "B1_RT2", "B1_RT3", "LIN_P19", "LIN_RT1")
OUTSIDE = ("F49", "T61", "T15")
COEF_CASES = ("C_RT1", "C_RT2", "C_RT3", "C_P19")
PADDED_CASES = GEOMETRY + OUTSIDE                      # COEF cases need the device's table: built by the GPU test (host: a surrogate)
SPECIALIZE_TWIN = "F34_B17"                            # also run under RD_K1_SPECIALIZE=0: the runtime-shape <3, 0, 0> at F 34, T 60

# ---- token-plan cases: (F, T) x length set --------------------------------------------------------------------------------------------
PLAN_SHAPES = {"P34x60": (34, 60), "P34x56": (34, 56), "P16x32": (16, 32), "P17x12": (17, 12), "P48x20": (48, 20), "P1x4": (1, 4),
               "P49x60": (49, 60), "P34x61": (34, 61)}            # the last two: outside the envelope, the generic path on a plan
PLAN_INSIDE = ("P34x60", "P34x56", "P16x32", "P17x12", "P48x20", "P1x4")
PLAN_OUTSIDE = ("P49x60", "P34x61")


def lengths_of(lset, T):
    """length sets in the manner of plan_layer_ref.LENGTHS, as functions of T (clipped to [0, T])"""
    raw = {"full": (T,) * 5,
           "ones": (1,) * 5,
           "zero": (T, 0, max(T // 2, 1), 0, 3),                  # zero-length samples own no row
           "ties": (5, T, 2, T, 5, 1, T - 1, 2, T),               # unsorted, with ties
           "l89": (8, 9, 9, 8, 9)}[lset]                          # both sides of a 32-column chunk edge (4 x 8 = 32)
    return tuple(int(min(max(l, 0), T)) for l in raw)


LSETS = ("full", "ones", "zero", "ties", "l89")
PLAN_CASES = [(s, l) for s in PLAN_INSIDE for l in LSETS] + [(s, "ties") for s in PLAN_OUTSIDE]

# A case whose gap-placed biases miss GATE_MARGIN (or the open share) gets another seed here -- never another margin.
SEED_BUMP = {("panel/M1", 1, 17, 1): 10}      # tests/panel_ref.py M1: the first seed at which the one row's last reduction index shows in z

VARIANTS = {"leftover_row": ("padded", "F34_B17"),       # the last leftover row of one sample dropped from dW1 and dW2
            "gate_neighbour": ("padded", "F34_B17"),     # one layer-1 gate taken from the neighbouring row
            "ssum_swap": ("padded", "F17"),              # ssum of two sensors exchanged
            "len_plus1": ("plan", ("P17x12", "l89")),    # one sample's length taken as L + 1 on the plan
            "drop_last_kc": ("padded", "F34_B16")}       # columns >= 32 floor(K / 32) dropped from layer 1's reduction, K % 32 == 16

# Bounds of the float64 tie.  Measured on the MI355X, maximum over the cases of a group with the worst case named
# (tests/test_sensor_stage_float64_gpu.py prints every figure with -s; profiles/sensor_stage_float64_errors.json holds all of them;
# z: max absolute error over z_scale; pe: max absolute error; gradients: max error over the tensor's float64 max-norm):
#             yardstick (RD_K1_FUSED=0)   fused, padded, bf16x3      fused, token plan          COEF, bf16x3         fp32 mode (generic)
#   z         6.89e-05  F47               6.84e-05  F47              5.79e-05  P17x12@ties      3.88e-05  C_P19      3.12e-06  F34_T56
#   pe        6.43e-08  F48               6.43e-08  F48              7.00e-08  P49x60@ties      6.13e-08  C_RT3      6.43e-08  F48
#   R_u       9.92e-06  F48               9.92e-06  F48              1.47e-05  P1x4@ones        1.03e-05  C_RT2      3.85e-07  F49
#   W1        1.79e-05  LIN_P19           1.79e-05  LIN_P19          1.35e-05  P34x60@ones      1.02e-05  C_P19      4.74e-07  LIN_P19
#   b1        7.14e-06  C_RT1             7.46e-06  F33              1.21e-05  P34x60@ones      7.15e-06  C_RT1      2.97e-07  F33
#   W2        1.90e-05  B1_RT1            1.90e-05  B1_RT1           1.64e-05  P17x12@full      7.41e-06  C_P19      3.32e-07  F31
#   b2        1.42e-07  F34_B17           4.42e-06  F1_B33           8.64e-06  P34x60@ones      2.88e-06  C_P19      1.36e-07  F49
# (The two paths split the same operands into the same three bf16 products and differ in summation order only, so most figures agree
# to three digits; the fused db comes out of the weight-gradient stream's constant ones tile, i.e. from split-bf16 dZ, the generic
# one from an fp32 column sum.)  The runtime-shape twin of F34_B17 / C_P19 is bit-equal to the specialised run.  No yardstick
# gradient error comes near 1e-4, so no bound is raised: RAISED is empty.
Z_ABS = {"bf16x3": 2e-5 * 6.0, "fp32": 2e-5}
PE_ABS = 2e-6
GRAD_REL = 2e-4
RAISED = {}                                              # tensor -> bound above GRAD_REL (2 x the yardstick's error)


def z_scale(zref):
    """1 where max |z_ref| is O(1) (within [1/8, 8]: z is compared in absolute terms), max |z_ref| otherwise"""
    m = float(np.abs(zref).max()) if zref.size else 1.0
    return 1.0 if 0.125 <= m <= 8.0 else m


def bound_of(mode):
    """name -> (metric, bound) of a compared tensor; "absz": max absolute error over z_scale(reference)"""
    def f(name):
        if name == "z":
            return ("absz", Z_ABS[mode])
        if name == "pe":
            return ("abs", PE_ABS)
        return ("rel", RAISED.get(name, GRAD_REL))
    return f


def in_envelope(F, T):
    """rd_k1_route.h k1_envelope at d_ob = 4"""
    K = 4 * T
    return F <= 48 and 16 <= K <= 240 and K % 16 == 0


def layout_numbers(F, T, B):
    """k1::make_layout / make_dw_plan (rd_k1_layout.h) restated: what the case table is chosen around"""
    q, rem = F // 32, F % 32
    per = 32 // rem if rem else 1
    S = B * q + (-(-B // per) if rem else 0)
    nct = 4 * T // 16
    nbn, nbk = (nct + 3) // 4, (nct + 4) // 4
    nslice = max(1, min(256 // (2 * nbn * nbk), S // 4))
    return dict(q=q, rem=rem, per=per, S=S, nct=nct, RT=-(-F // 16), nkc=-(-4 * T // 32), nslice=nslice)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _observed(rng, F, T, lengths, pattern):
    """bool [T, B, F]: which (step, sample, sensor) cells hold an observation; none at steps >= the sample's length"""
    B = len(lengths)
    valid = np.arange(T)[:, None] < np.asarray(lengths)[None, :]
    obs = (rng.random((T, B, F)) < 0.5) & valid[:, :, None]
    if pattern == "lin":
        # sample 0: no observation at all (lin = 0); samples 1 .. 4: the last observation at step 0, 7, 8, T - 1 (their lengths are
        # set to match in _lengths); one sensor unobserved in every sample
        obs[:, 0, :] = False
        for b, last in zip(range(1, 5), (0, 7, 8, T - 1)):
            obs[last + 1:, b, :] = False
            obs[last, b, 0] = True
        obs[:, :, min(2, F - 1)] = False
    return obs


def _lengths(rng, T, B, pattern):
    L = rng.integers(1, T + 1, size=B)
    L[0] = T
    if pattern == "lin":
        L[0] = max(T // 2, 1)
        for b, last in zip(range(1, 5), (0, 7, 8, T - 1)):
            L[b] = last + 1
    return L.astype(np.int64)


def _rng(*key):
    return np.random.default_rng([zlib.crc32(repr(key).encode()), SEED_BUMP.get(key, 0)])


def gap_bias(P):
    """fp32 [K]: -(midpoint of the widest gap inside the 25 % .. 75 % rank range of the distinct values of each column of P [rows, K]
    and 0.0)"""
    out = np.empty(P.shape[1], dtype=np.float32)
    for n in range(P.shape[1]):
        v = np.unique(np.concatenate([P[:, n], [0.0]]))
        m = len(v)
        assert m >= 2, "a column with one distinct value has no gap"
        lo, hi = (m - 1) // 4, -(-3 * (m - 1) // 4)
        i = lo + int(np.argmax(v[lo + 1:hi + 1] - v[lo:hi]))
        out[n] = -(v[i] + v[i + 1]) / 2.0
    return out


def _embed(c):
    """X [B, F, K] float64"""
    T, B, F = c["T"], c["B"], c["F"]
    v = c["src"][:, :, :F].astype(np.float64)                                    # [T, B, F]
    x = np.maximum(v[:, :, :, None] * c["R_u"].astype(np.float64).reshape(F, D_OB)[None, None], 0.0)     # [T, B, F, d]
    return x.transpose(1, 2, 0, 3).reshape(B, F, T * D_OB)


def _scales(c, ssum=None):
    """s1, s2 [B, F] float64: ssum[f], or the rows of the coefficient table"""
    if c["coef"] is not None:
        return c["coef"][0].astype(np.float64), c["coef"][1].astype(np.float64)
    s = np.broadcast_to((c["ssum"] if ssum is None else ssum).astype(np.float64)[None, :], (c["B"], c["F"]))
    return s, s


def make_case(name, F, T, lengths, pattern, layout, coef=None, ssum=None):
    """Inputs of one case.  coef [2, B, F] / ssum [F] fp32: data read back from the device (COEF cases); otherwise ssum is drawn here.
    b1, b2 are gap-placed (fp32) from the float64 products."""
    B = len(lengths)
    assert B * F <= MAX_ROWS and B <= 40
    K = T * D_OB
    key = (name, F, T, B)
    rng = _rng(*key)
    L = np.asarray(lengths, dtype=np.int64)
    obs = _observed(rng, F, T, L, pattern)
    vals = rng.standard_normal((T, B, F)) * obs
    src = np.concatenate([vals, obs.astype(np.float64)], axis=-1).astype(np.float32)
    valid = np.arange(T)[:, None] < L[None, :]
    times = (np.cumsum(rng.random((T, B)) + 0.01, axis=0) * valid).astype(np.float32)
    fill = float(np.clip(L, 0, T).sum()) / (T * B)                               # share of live steps: short samples get a larger R_u
    R_u = (1.5 / np.sqrt(fill) * rng.standard_normal((1, F * D_OB))).astype(np.float32)
    W1 = (rng.standard_normal((K, K)) / np.sqrt(K)).astype(np.float32)
    W2 = (rng.standard_normal((K, K)) / np.sqrt(K)).astype(np.float32)
    drawn = rng.uniform(0.5, 1.5, size=F).astype(np.float32)
    dz = rng.standard_normal((T, B, F * D_OB + D_PE)).astype(np.float32)
    c = dict(name=name, F=F, T=T, B=B, K=K, D=F * D_OB + D_PE, lengths=L, pattern=pattern, layout=layout, src=src, times=times,
             R_u=R_u, W1=W1, W2=W2, ssum=drawn if ssum is None else np.asarray(ssum, dtype=np.float32),
             coef=None if coef is None else np.asarray(coef, dtype=np.float32), dz=dz, plan=plan_ref(L, T),
             envelope=in_envelope(F, T))
    assert c["coef"] is None or c["coef"].shape == (2, B, F)
    # the X gate is exact: every non-zero product is a normal fp32 number
    prod = np.abs(src[:, :, :F, None] * R_u.reshape(F, D_OB)[None, None])
    assert not ((prod > 0) & (prod < np.finfo(np.float32).tiny)).any()
    X = _embed(c)
    s1, _ = _scales(c)
    P1 = X @ W1.astype(np.float64).T
    c["b1"] = gap_bias(P1.reshape(B * F, K))
    Y1 = np.maximum(P1 + c["b1"].astype(np.float64), 0.0) * s1[:, :, None]
    c["b2"] = gap_bias((Y1 @ W2.astype(np.float64).T).reshape(B * F, K))
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """a padded-layout case of SHAPES (COEF cases: with the host's surrogate table -- the GPU test builds them from the device's)"""
    F, T, B, pattern = SHAPES[name]
    lengths = _lengths(_rng("lengths", name), T, B, pattern)
    coef = surrogate_coef(name) if name in COEF_CASES else None
    return make_case(name, F, T, lengths, pattern, "padded", coef=coef)


@functools.lru_cache(maxsize=None)
def plan_case(shape, lset):
    F, T = PLAN_SHAPES[shape]
    return make_case("%s@%s" % (shape, lset), F, T, lengths_of(lset, T), "dense", "plan")


def surrogate_coef(name):
    """[2, B, F] fp32 stand-in for rd_msgpass_coef_table's output on the host: coefficients of the table's kind (a tenth of them zero:
    every edge into the sensor dropped), so the host conditions run the same code as the GPU test's device-made table"""
    F, T, B, _ = SHAPES[name]
    rng = _rng("coef", name)
    return (rng.uniform(0.3, 1.7, size=(2, B, F)) * (rng.random((2, B, F)) >= 0.1)).astype(np.float32)


# ---- layouts --------------------------------------------------------------------------------------------------------------------------
def starts_of(pl):
    """first plan row of every SAMPLE (caller's order)"""
    return pl["off"][pl["rank"]]


def to_plan(padded, starts, lengths, mlive):
    """[T, B, D] -> [M_live, D] plan order (live steps only)"""
    out = np.zeros((mlive, padded.shape[2]), dtype=padded.dtype)
    for b, (s, n) in enumerate(zip(starts, lengths)):
        out[s:s + n] = padded[:n, b]
    return out


def to_padded(rows, starts, lengths, T):
    """[M, D] plan order -> [T, B, D] with zeros at padded steps"""
    out = np.zeros((T, len(lengths), rows.shape[1]), dtype=rows.dtype)
    for b, (s, n) in enumerate(zip(starts, lengths)):
        out[:n, b] = rows[s:s + n]
    return out


def live_dz(c, lengths=None):
    """dz as the reference sees it, [T, B, D]: on a plan the device holds to_plan(c["dz"]) and steps >= length carry no gradient.
    `lengths` (variant len_plus1): the lengths a wrong kernel would walk the same plan rows with."""
    if c["layout"] == "padded":
        return c["dz"]
    pl = c["plan"]
    st = starts_of(pl)
    rows = to_plan(c["dz"], st, c["lengths"], pl["mlive"])
    rows = np.concatenate([rows, np.zeros((1, rows.shape[1]), rows.dtype)])       # the row behind the last live one
    return to_padded(rows, st, c["lengths"] if lengths is None else lengths, c["T"])


# ---- the float64 reference --------------------------------------------------------------------------------------------------------------
def pe_reference(times, T):
    """[T, B, 16] float64: sine and cosine, in float64, of the fp32 angle oracle/restatement.py positional_encoding forms"""
    ts = torch.tensor(T ** np.linspace(0, 1, D_PE // 2), dtype=torch.float32)
    ang = (torch.from_numpy(times).unsqueeze(2) / ts[None, None, :]).double().numpy()
    return np.concatenate([np.sin(ang), np.cos(ang)], axis=-1)


def evaluate(c, variant=None):
    """{z [T, B, 4F], pe [T, B, 16], mask [B, T], R_u, W1, b1, W2, b2 (gradients), pre1, pre2 [B, F, K]} in float64 on the padded
    layout (compared(): what the device comparison holds to bounds, live rows on a plan)."""
    T, B, F, K = c["T"], c["B"], c["F"], c["K"]
    W1, W2 = c["W1"].astype(np.float64), c["W2"].astype(np.float64)
    b1, b2 = c["b1"].astype(np.float64), c["b2"].astype(np.float64)
    ssum = c["ssum"]
    if variant == "ssum_swap":
        ssum = ssum.copy()
        ssum[[0, 1]] = ssum[[1, 0]]
    s1, s2 = _scales(c, ssum)
    X = _embed(c)
    Xin = X
    if variant == "drop_last_kc":                          # the final reduction step of layer 1's product never runs
        assert K % 32 == 16
        Xin = X.copy()
        Xin[:, :, 32 * (K // 32):] = 0.0
    if variant == "drop_last_k":                           # tests/panel_ref.py: the last reduction index of both products never runs
        Xin = X.copy()
        Xin[:, :, K - 1] = 0.0
    pre1 = Xin @ W1.T + b1
    g1 = pre1 > 0
    if variant == "gate_neighbour":                        # row (b, f) of one column gated by row (b, f + 1)'s bit
        differ = g1[:, :-1] != g1[:, 1:]
        score = np.where(differ, np.abs(pre1[:, :-1]) * s1[:, :-1, None], -1.0)
        b_, f_, n_ = np.unravel_index(int(np.argmax(score)), score.shape)
        g1 = g1.copy()
        g1[b_, f_, n_] = g1[b_, f_ + 1, n_]
    Y1 = np.where(g1, pre1, 0.0) * s1[:, :, None]
    Y1in = Y1
    if variant == "drop_last_k":
        Y1in = Y1.copy()
        Y1in[:, :, K - 1] = 0.0
    pre2 = Y1in @ W2.T + b2
    g2 = pre2 > 0
    Y2 = np.where(g2, pre2, 0.0) * s2[:, :, None]
    z = Y2.reshape(B, F, T, D_OB).transpose(2, 0, 1, 3).reshape(T, B, F * D_OB)
    # backward
    lengths = None
    if variant == "len_plus1":
        lengths = c["lengths"].copy()
        b_ = int(c["plan"]["order"][B - 2])                # the last sample but one in plan order: its row L is the next sample's row 0
        assert lengths[b_] < T
        lengths[b_] += 1
    dz = live_dz(c, lengths)[:, :, :F * D_OB].astype(np.float64)
    dY2 = dz.reshape(T, B, F, D_OB).transpose(1, 2, 0, 3).reshape(B, F, K)
    dP2 = dY2 * s2[:, :, None] * g2
    dP1 = (dP2 @ W2) * s1[:, :, None] * g1
    dX = dP1 @ W1
    keep = np.ones((B, F, 1))
    if variant == "leftover_row":
        keep[B - 1, F - 1] = 0.0
    dW2 = np.einsum("bfn,bfk->nk", dP2 * keep, Y1)
    dW1 = np.einsum("bfn,bfk->nk", dP1 * keep, X)
    v = c["src"][:, :, :F].astype(np.float64)                                    # [T, B, F]
    dXs = (dX * (X > 0)).reshape(B, F, T, D_OB)
    dRu = np.einsum("bftc,tbf->fc", dXs, v).reshape(1, F * D_OB)
    return dict(z=z, pe=pe_reference(c["times"], T), mask=O2.padding_mask(c["lengths"], T), R_u=dRu, W1=dW1, b1=dP1.sum((0, 1)),
                W2=dW2, b2=dP2.sum((0, 1)), pre1=pre1, pre2=pre2)


_REF = {}


def reference(c, variant=None):
    """evaluate(), computed once per (case, variant) and shared: callers must not modify it"""
    key = (c["name"], c["layout"], variant, c["ssum"].tobytes(), None if c["coef"] is None else c["coef"].tobytes())
    if key not in _REF:
        _REF[key] = evaluate(c, variant)
    return _REF[key]


def compared(c, ref):
    """the tensors the device comparison holds to bounds: z and pe on live rows in plan order where the case runs on a plan"""
    out = {k: ref[k] for k in GRAD_NAMES}
    if c["layout"] == "plan":
        pl = c["plan"]
        st = starts_of(pl)
        out["z"] = to_plan(ref["z"], st, c["lengths"], pl["mlive"])
        out["pe"] = to_plan(ref["pe"], st, c["lengths"], pl["mlive"])
    else:
        out["z"], out["pe"] = ref["z"], ref["pe"]
    return out


def error_of(name, got, ref, mode):
    """(error in the tensor's metric, bound)"""
    metric, bound = bound_of(mode)(name)
    a, r = np.asarray(got, dtype=np.float64), ref
    assert a.shape == r.shape, (name, a.shape, r.shape)
    e = float(np.abs(a - r).max()) if a.size else 0.0
    if metric == "rel":
        e /= float(np.abs(r).max()) + 1e-30
    elif metric == "absz":
        e /= z_scale(r)
    return e, bound
