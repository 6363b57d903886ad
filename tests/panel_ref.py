"""TEST INFRASTRUCTURE ONLY -- the panel products of raindrop_amd/csrc/rd_gemm.hip (k_gemm_panel 64 x 128, k_gemm_panel_wide
128 x 256, k_gemm_panel_pc 128 x 128 producer / consumer) across the places of their reduction loop, row halves and tile maps
that the cost model never selects at the suite's shapes: case table, forced forms, routes.

Used by tests/test_panel_ref_host.py (the route table against rd_debug_gemm_route, the conditions on the reference alone; no GPU)
and tests/test_panel_float64_gpu.py (every case in every forced form against float64).

Reference, inputs and bounds are those of tests/sensor_stage_ref.py, imported: the generic sensor stage runs four panel products
([B F, K] x [K, K], K = 4 T: two forward with bias, ReLU, row scale and -- the second -- the d_ob = 4 scatter, two input gradients,
the first with the gate mask and row scale), so a case is a sensor-stage case (F, T, B) with M = B F rows and K = N = 4 T, run under
a forced form (RD_PANEL_WIDE / RD_PANEL_PC, read per call) and, inside the fused kernels' envelope, under RD_K1_FUSED=0.  Gates are
decisive (GATE_MARGIN), so z is held to 2e-5 x 6 and every gradient to 2e-4 of its float64 max-norm with no entry exempt
(sensor_stage_ref.bound_of, unchanged).  The weight gradients of the stage are split-K products with row sums -- never a panel
candidate -- and get the same tie on the way.

What a case is there for (nch = ceil(K / 64) chunks; a chunk is two 32-k weight tiles; small: two wave groups take even / odd chunks):
    K64    nch 1: group 1 of the small form owns no chunk          K68    nch 2, tail 4: the last chunk's second weight tile does not
    K96    tail exactly 32                                                exist (re-read, against zero A columns); N % 16 = 4
    K100   tail 36: the second tile exists, 4 columns deep          K128   two full chunks
    K160   nch 3, odd, the last half a chunk                        K192   nch 3, odd, full
    K260   nch 5; N > 256: two column blocks in the wide form, the second 4 columns deep (three in the others)
    M1 .. M129   row counts 1, 63, 64, 65, 127, 128, 129 at K = 68: the second half-tile of wide / pc empty, one row deep, full
    TILES  520 x 260: 27 / 10 / 15 tiles -- more than 8 and no multiple of 8 under the XCD map (M1: one tile, seven workgroups idle)
    COEF   row scales per graph row (rs_period = M)                 PLAN   the second product's scatter on a registered token plan,
                                                                           one sample of length 1 and one of full length
The encoder-layer case (ENC): D = 84, nhid = 136, T = 33, B = 5 -- 165 rows (a second half-tile of 37), K = 84 (nch 2, tail 20),
136 (nch 3, tail 8), 252 (nch 4, tail 28) -- for the dropout + residual and posmask + cscale epilogues of the forced forms;
linear1.bias is gap-placed so that no FFN gate can flip."""
import functools

import numpy as np
import torch

from oracle import restatement as O2
from tests import dropout_ref as DR
from tests import sensor_stage_ref as SR

FORMS = {"small": (64, 128, 8), "wide": (128, 256, 4), "pc": (128, 128, 4)}       # workgroup tile, hi / lo planes in LDS
PANEL_NAME = {"small": "k_gemm_panel", "wide": "k_gemm_panel_wide", "pc": "k_gemm_panel_pc"}
FORCE = {"small": {"RD_PANEL_WIDE": "0", "RD_PANEL_PC": "0"}, "wide": {"RD_PANEL_WIDE": "1", "RD_PANEL_PC": "0"},
         "pc": {"RD_PANEL_PC": "1"}}
X3 = "k_gemm_bf16x3_"
MODE = "bf16x3"

# ---- cases: name -> (F, T, B, kind) --------------------------------------------------------------------------------------------------
CASES = {
    "K64": (34, 16, 5, "padded"), "K68": (34, 17, 5, "padded"), "K96": (34, 24, 5, "padded"), "K100": (34, 25, 5, "padded"),
    "K128": (34, 32, 5, "padded"), "K160": (34, 40, 5, "padded"), "K192": (34, 48, 5, "padded"), "K260": (34, 65, 5, "padded"),
    "M1": (1, 17, 1, "padded"), "M63": (21, 17, 3, "padded"), "M64": (32, 17, 2, "padded"), "M65": (13, 17, 5, "padded"),
    "M127": (127, 17, 1, "padded"), "M128": (32, 17, 4, "padded"), "M129": (43, 17, 3, "padded"),
    "TILES": (40, 65, 13, "padded"),
    "COEF": (34, 17, 5, "coef"),
    "PLAN": (34, 17, 5, "plan"),
}
PLAN_LENGTHS = {"PLAN": (17, 1, 5, 16, 9)}               # full length, length 1, and three in between (unsorted)
# the route the table states: every product of every case has K >= 64 and runs on the forced form's kernel
ROUTE = {(name, form): PANEL_NAME[form] for name in CASES for form in FORMS}
# by hand: (rows, columns) and the tile counts of the cases chosen for the tile map -- small, wide, pc
TILE_COUNTS = {"M1": (1, 68, (1, 1, 1)), "K260": (170, 260, (9, 4, 6)), "TILES": (520, 260, (27, 10, 15))}
ROW_SUBSET = {"case": "K68", "samples": (1, 3)}          # 170 rows > every TM; the second call: 68 rows of samples 1 and 3
GUARD_CASES = ("K68", "PLAN")                            # the write-side guard: padded layout and token plan

# A case whose gap-placed biases miss GATE_MARGIN, or whose edges do not show above the bound, gets another seed in
# sensor_stage_ref.SEED_BUMP (key ("panel/" + name, F, T, B)) -- never another margin.  M1 has one.


def cdiv(a, b):
    return -(-a // b)


def dims(name):
    """(M, K) of a case's four products"""
    F, T, B, _ = CASES[name]
    return B * F, T * SR.D_OB


def tiles(name, form):
    M, K = dims(name)
    tm, tn, _ = FORMS[form]
    return cdiv(M, tm) * cdiv(K, tn)


def launch(name, form):
    """(kernel name, grid x, dynamic LDS bytes) of every product of the case in the form -- rd_gemm.hip gemm_route restated"""
    tm, tn, planes = FORMS[form]
    return ROUTE[(name, form)], 8 * cdiv(tiles(name, form), 8), planes * tm * 80 * 2 + 4 * tn


def conditions(name):
    """what the reduction loop sees at the case's K"""
    _, K = dims(name)
    return dict(nch=cdiv(K, 64), tail=K % 64, nkc=cdiv(K, 32))


def _coef(name):
    """[2, B, F] fp32 per-row scales of the table's kind (a tenth zero) -- to the panel kernels a row-scale array of period M"""
    F, T, B, _ = CASES[name]
    rng = SR._rng("panel-coef", name)
    return (rng.uniform(0.3, 1.7, size=(2, B, F)) * (rng.random((2, B, F)) >= 0.1)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """the sensor-stage case (sensor_stage_ref.make_case) behind a name of CASES"""
    F, T, B, kind = CASES[name]
    tag = "panel/" + name
    if kind == "plan":
        assert len(PLAN_LENGTHS[name]) == B
        return SR.make_case(tag, F, T, PLAN_LENGTHS[name], "dense", "plan")
    lengths = SR._lengths(SR._rng("lengths", tag), T, B, "dense")
    return SR.make_case(tag, F, T, lengths, "dense", "padded", coef=_coef(name) if kind == "coef" else None)


def subset_case(c, samples):
    """c restricted to `samples` (padded layout) with c's OWN biases: the same products over fewer rows"""
    idx = list(samples)
    s = dict(c)
    s.update(name=c["name"] + "/rows", B=len(idx), lengths=c["lengths"][idx], src=np.ascontiguousarray(c["src"][:, idx]),
             times=np.ascontiguousarray(c["times"][:, idx]), dz=np.ascontiguousarray(c["dz"][:, idx]),
             coef=None if c["coef"] is None else np.ascontiguousarray(c["coef"][:, idx]))
    return s


# ---- the edges, on the reference alone ---------------------------------------------------------------------------------------------------
def edge_margins(c):
    """How far three edge errors move z, in units of its bound (each must exceed 1): the last reduction index of both products
    dropped, the last graph row zeroed, any one of the last four output columns (step T - 1: the whole ragged column block of K = 260;
    samples of full length) zeroed -- the smallest of the four (under 8 rows, where a column can be all closed gates: the largest)."""
    ref = SR.reference(c)
    z = ref["z"]
    _, bound = SR.bound_of(MODE)("z")
    unit = bound * SR.z_scale(z)
    F, T, B = c["F"], c["T"], c["B"]
    full = np.flatnonzero(c["lengths"] == T)
    assert len(full), "no sample of full length"
    steps = int(c["lengths"][B - 1])                      # on a plan the last sample's rows exist for its live steps only
    return dict(last_k=float(np.abs(SR.reference(c, "drop_last_k")["z"] - z).max()) / unit,
                last_row=float(np.abs(z[:steps, B - 1, SR.D_OB * (F - 1):]).max()) / unit,
                last_col=(min if B * F >= 8 else max)(float(np.abs(z[T - 1][full][:, k::SR.D_OB]).max()) for k in range(SR.D_OB)) / unit)


# ---- the encoder layer in the forced forms ---------------------------------------------------------------------------------------------
ENC = dict(T=33, B=5, F=17, nhead=2, layer=0)             # D = 84, nhid = 136
ENC_P = (0.0, DR.P_DROP)
ENC_FORMS = ("wide", "pc")


def enc_products():
    """(M, N, K) of the layer's eight dense products: four forward, four input gradients"""
    M, D, H = ENC["T"] * ENC["B"], 4 * ENC["F"] + 16, 8 * ENC["F"]
    fwd = [(M, 3 * D, D), (M, D, D), (M, H, D), (M, D, H)]
    return fwd + [(M, k, n) for _, n, k in fwd]


def _enc_forward(c, p, p_drop, gates=None):
    xr = c["x"].double().requires_grad_(True)
    pr = {("L." + n): t.double().requires_grad_(True) for n, t in p.items()}
    hook = None
    if p_drop > 0:
        hook = DR.DropHook(DR.Masks(DR.SEED, p_drop, c["T"], c["B"]).encoder(ENC["layer"], c["nhead"], c["D"], c["nhid"]))
    y = O2.encoder_layer(xr, c["mask"], pr, "L.", c["nhead"], drop=hook, gates=gates)
    return xr, pr, y


@functools.lru_cache(maxsize=None)
def enc_case():
    """dropout_ref.enc_case at the shape, with linear1.bias placed in the widest gap (sensor_stage_ref.gap_bias) of the columns of
    LN1(..) W1^T over the rows of BOTH runs (p = 0 and p = 0.2): |pre| >= GATE_MARGIN in either, no FFN gate can flip"""
    base = DR.enc_case(ENC["T"], ENC["B"], ENC["F"], ENC["nhead"])
    c = dict(base)
    p = dict(base["p"])
    p["linear1.bias"] = torch.zeros_like(p["linear1.bias"])
    rows = []
    for pd in ENC_P:
        g = {}
        with torch.no_grad():
            _enc_forward(c, p, pd, g)
        rows.append(g["L.linear1"].numpy().reshape(-1, c["nhid"]))
    p["linear1.bias"] = torch.from_numpy(SR.gap_bias(np.concatenate(rows)))
    c["p"] = p
    return c


@functools.lru_cache(maxsize=None)
def enc_reference(p_drop):
    """oracle/restatement.py encoder_layer in float64 with the host masks of tests/dropout_ref.py (none at p = 0): the output, all
    13 gradients and the FFN's pre-activations"""
    c = enc_case()
    g = {}
    xr, pr, y = _enc_forward(c, c["p"], p_drop, g)
    grads = torch.autograd.grad(y, [xr] + [pr["L." + n] for n in DR.ENC_NAMES], c["dy"].double())
    res = {"y": y.detach().numpy()}
    res.update((n, t.numpy()) for n, t in zip(("x",) + DR.ENC_NAMES, grads))
    return res, g["L.linear1"].numpy()


# ---- the one-product bf16 mode ---------------------------------------------------------------------------------------------------------
# A float64 tie at stage level means nothing there (operands are rounded to bf16: errors of 1e-3 .. 1e-2 against float64, and the
# float64-placed biases no longer decide the gates).  What the mode is held to instead:
#   * a case of its own per name (case16): the same inputs with b1, b2 gap-placed from the products of the bf16-ROUNDED operands, so
#     that |pre| >= GATE_MARGIN holds in the arithmetic the kernels run (test_panel_ref_host.py);
#   * reference (evaluate16): float64 sums of products of bf16-rounded operands -- X, W1, Y1 (from fp32), W2 forward; dZ2, dZ1 backward
#     -- as tests/test_gemm_tiles_gpu.py ties its one-product products (operand.bfloat16().double());
#   * z, element by element: the split-bf16 bound 2e-5 x 6 x z_scale (fp32 accumulation of exact products is no worse than that) plus
#     ONE flipped bf16 rounding of Y1 in the element's row: s2[r] max_k ulp_bf16(Y1[r, k]) |W2[n, k]|.  The device's Y1 differs from
#     the reference's by fp32 summation order (1e-7), which moves a value across a bf16 rounding boundary in about one row of a
#     hundred; two in one element are not allowed for;
#   * the three forms pairwise on the same inputs: 4 x the largest difference, over the cases and both forward products, between
#     the two fp32 summation orders of the same bf16-rounded products (chunk order | even / odd 64-k chunks in two accumulator sets,
#     32-k steps as the MFMA takes them) -- PAIR_SUM, computed here on the CPU -- plus the same one-flip term; PE and mask bit-equal;
#   * gradients: relative L2 2e-2 and max-norm 0.25 against evaluate16, the bound test_sensor_stage_vs_oracle applies in the bf16
#     modes (_grad_close); a flipped rounding of dZ2, dZ1 or Y1 moves single entries by ~2^-8 and stays far below it.
def bf16(a):
    """round to bf16 (nearest even, as the kernels' conversion), back in float64"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().double().numpy()


def ulp_bf16(a):
    """spacing of bf16 numbers at |a| (0 at 0)"""
    m = np.abs(a)
    return np.where(m > 0, 2.0 ** (np.floor(np.log2(np.where(m > 0, m, 1.0))) - 7), 0.0)


def _x32(c):
    """X as the device forms it: relu of the fp32 product src * R_u, [B, F, K]"""
    T, B, F = c["T"], c["B"], c["F"]
    x = np.maximum(c["src"][:, :, :F, None] * c["R_u"].reshape(F, SR.D_OB)[None, None], np.float32(0))
    assert x.dtype == np.float32
    return x.transpose(1, 2, 0, 3).reshape(B, F, T * SR.D_OB)


@functools.lru_cache(maxsize=None)
def case16(name):
    c = dict(case(name))
    B, F, K = c["B"], c["F"], c["K"]
    s1, _ = SR._scales(c)
    P1 = bf16(_x32(c)) @ bf16(c["W1"]).T
    c["b1"] = SR.gap_bias(P1.reshape(B * F, K))
    Y1 = (np.maximum(P1 + c["b1"].astype(np.float64), 0.0) * s1[:, :, None]).astype(np.float32)
    c["b2"] = SR.gap_bias((bf16(Y1) @ bf16(c["W2"]).T).reshape(B * F, K))
    c["name"] = c["name"] + "/bf16"
    return c


def _to_z(c, Y):
    return Y.reshape(c["B"], c["F"], c["T"], SR.D_OB).transpose(2, 0, 1, 3).reshape(c["T"], c["B"], c["F"] * SR.D_OB)


def evaluate16(c, drop_last_k=False):
    """as sensor_stage_ref.evaluate with every product's operands rounded to bf16; plus zflip [T, B, 4F], the one-flip term of z"""
    T, B, F, K = c["T"], c["B"], c["F"], c["K"]
    W1, W2 = bf16(c["W1"]), bf16(c["W2"])
    b1, b2 = c["b1"].astype(np.float64), c["b2"].astype(np.float64)
    s1, s2 = SR._scales(c)
    X32 = _x32(c)
    X = bf16(X32)
    Xin = X.copy()
    if drop_last_k:
        Xin[:, :, K - 1] = 0.0
    pre1 = Xin @ W1.T + b1
    g1 = pre1 > 0
    Y1 = bf16((np.where(g1, pre1, 0.0) * s1[:, :, None]).astype(np.float32))
    Y1in = Y1.copy()
    if drop_last_k:
        Y1in[:, :, K - 1] = 0.0
    pre2 = Y1in @ W2.T + b2
    g2 = pre2 > 0
    z = _to_z(c, np.where(g2, pre2, 0.0) * s2[:, :, None])
    flip = np.zeros((B, F, K))
    U = ulp_bf16(Y1)
    for k in range(K):
        np.maximum(flip, U[:, :, k:k + 1] * np.abs(W2[:, k])[None, None, :], out=flip)
    dz = SR.live_dz(c)[:, :, :F * SR.D_OB].astype(np.float64)
    dY2 = dz.reshape(T, B, F, SR.D_OB).transpose(1, 2, 0, 3).reshape(B, F, K)
    dP2 = bf16((dY2 * s2[:, :, None] * g2).astype(np.float32))
    dP1 = bf16(((dP2 @ W2) * s1[:, :, None] * g1).astype(np.float32))
    dX = dP1 @ W1
    v = c["src"][:, :, :F].astype(np.float64)
    dRu = np.einsum("bftc,tbf->fc", (dX * (X32 > 0)).reshape(B, F, T, SR.D_OB), v).reshape(1, F * SR.D_OB)
    return dict(z=z, zflip=_to_z(c, flip * s2[:, :, None]), pe=SR.pe_reference(c["times"], T), mask=O2.padding_mask(c["lengths"], T),
                R_u=dRu, W1=np.einsum("bfn,bfk->nk", dP1, X), b1=dP1.sum((0, 1)), W2=np.einsum("bfn,bfk->nk", dP2, Y1),
                b2=dP2.sum((0, 1)), pre1=pre1, pre2=pre2, X=X, Y1=Y1)


_REF16 = {}


def reference16(name):
    if name not in _REF16:
        _REF16[name] = evaluate16(case16(name))
    return _REF16[name]


def compared16(name):
    """z, zflip, pe and the gradients as the device comparison holds them (live rows in plan order on a plan)"""
    c, r = case16(name), reference16(name)
    out = SR.compared(c, r)
    out["zflip"] = r["zflip"]
    if c["layout"] == "plan":
        out["zflip"] = SR.to_plan(r["zflip"], SR.starts_of(c["plan"]), c["lengths"], c["plan"]["mlive"])
    return out


def z_bound16(name):
    """element-wise bound of z in the one-product mode, in compared16's layout"""
    cmp_ = compared16(name)
    return SR.Z_ABS["bf16x3"] * SR.z_scale(cmp_["z"]) + cmp_["zflip"]


def _sum_orders(A, Wt):
    """fp32 sums of the products A [M, K] Wt [N, K]^T (bf16 values) over 32-k steps: in chunk order, and with even / odd 64-k chunks
    in two accumulators added at the end"""
    A32, W32 = A.astype(np.float32), Wt.astype(np.float32)
    K = A.shape[1]
    seq = np.zeros((A.shape[0], Wt.shape[0]), np.float32)
    two = [seq.copy(), seq.copy()]
    for k0 in range(0, K, 32):
        p = (A32[:, k0:k0 + 32].astype(np.float64) @ W32[:, k0:k0 + 32].astype(np.float64).T)
        seq = (seq.astype(np.float64) + p).astype(np.float32)          # one MFMA step: exact products, one rounding of the sum
        g = (k0 // 64) & 1
        two[g] = (two[g].astype(np.float64) + p).astype(np.float32)
    return seq, two[0] + two[1]


@functools.lru_cache(maxsize=None)
def pair_sum():
    """PAIR_SUM: 4 x the largest |chunk order - even / odd order| over the cases and both forward products, and the per-case figures"""
    per = {}
    for name in CASES:
        c, r = case16(name), reference16(name)
        M, K = c["B"] * c["F"], c["K"]
        d = 0.0
        for A, W in ((r["X"], c["W1"]), (r["Y1"], c["W2"])):
            a, b = _sum_orders(A.reshape(M, K), bf16(W))
            d = max(d, float(np.abs(a.astype(np.float64) - b).max()))
        per[name] = d
    return 4.0 * max(per.values()), per
