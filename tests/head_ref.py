"""TEST INFRASTRUCTURE ONLY -- the fused classifier head (rd_head.hip: k_head_rows<1,12,3> / <1,16,4>, plain and CRIT, k_head_wgrad,
behind rd_head_train / rd_head_train_crit / rd_head_forward / rd_head_backward): case table, inputs, float64 reference and bounds.

Used by tests/test_head_ref_host.py (conditions on the reference alone, no GPU) and tests/test_head_float64_gpu.py (every case through
the C-ABI against this reference).

Reference (numpy; `evaluate`): code/models_rd.py:366-385 and code/Raindrop.py:255,322 on the head's own inputs r [T,B,D], lengths [B]
(the mask is their prefix mask), stat [B,ds], emb_w [Fe,ds], emb_b [Fe], w0 [dh,dh], b0 [dh], w2 [C,dh], b2 [C], y [B], dh = D + Fe:
    agg    = sum_t r[t] keep[t] / (len + 1),   keep[t,b] = t < len[b]
    feat   = [agg | stat emb_w^T + emb_b]
    logits = w2 relu(w0 feat + b0) + b2
    loss   = mean cross entropy ("plain"), torch's CrossEntropyLoss(weight, label_smoothing = EPS), mean reduction ("crit"), or none
             at all: a cotangent on the logits from the caller ("cot", rd_head_backward)
and the chain rule written out by hand for dr, dW0, db0, dW2, db2, d emb_w, d emb_b.  On the token plan r and dr are [M_live, D] in
plan order (tests/helpers.plan_ref): `rows_of`.  A zero-length sample owns no row, its agg is 0 and it still reaches every parameter
gradient through b0 and the static block.  Every reduction is a running sum in the working precision (`_mm`, `_seq_sum`), so the
SAME code in float32 is the yardstick: what fp32 arithmetic alone costs this chain.  tests/test_head_ref_host.py holds the float64
evaluation to torch autograd and to a central finite difference.

Decisive gates.  ReLU is discontinuous in the sign of the pre-activation, so no case leaves one at rounding distance from zero: b0[j]
is minus the midpoint of the widest gap between the sorted float64 values (w0 feat)[b, j] over the B rows (any gap between neighbours
leaves a row open and a row shut); at B = 1 it is -(w0 feat)[0, j] +/- B1_OFFSET with alternating sign.  After the rounding of b0 to
fp32 every |pre| >= GATE_MARGIN = 1e-3 (absolute; the convention of tests/sensor_stage_ref.py) -- tests/test_head_ref_host.py asserts
it for every case, and a case that misses it gets another seed through SEED_BUMP, never another margin.  No entry of any tensor is
exempt from the comparison.

Bounds (`bound_of`).  Ceilings: the project's figures for the head (test_fused_head_against_float64), 1e-6 on the loss relative to
max(1, |loss|), 2e-5 of the float64 max-norm on the logits and every gradient.  Working bound per tensor, case and loss form:
min(ceiling, 4 x yardstick), the yardstick being the float32 evaluation's error against the float64 one, never taken below 8 fp32 ulps
of the tensor's max-norm (a one-term sum has a yardstick of zero; the kernel's other order of additions must not fail on it).  4 x is
the margin of tests/beta_operator_ref.py, for the same reason: the kernel's fixed-order sums (lanes, then waves; 256-row chunks) are
not numpy's.  No bound reads a device number.  Wherever the float64 reference is exactly zero (dr at the padded steps of the padded
layout, everything a zero cotangent gives, everything at C = 1) the result must be exactly zero."""
import functools
import zlib

import numpy as np

from tests.helpers import plan_ref

GATE_MARGIN = 1e-3                                       # tests/sensor_stage_ref.py's
B1_OFFSET = 0.05
EPS = 0.1                                                # label smoothing of the "crit" form
FORMS = ("plain", "crit", "cot")
GRADS = ("dr", "dW0", "db0", "dW2", "db2", "demb_w", "demb_b")
COMPARED = ("logits",) + GRADS                           # and the loss
CEILING, LOSS_CEILING = 2e-5, 1e-6
YARD_FACTOR, FLOOR_ULPS = 4.0, 8
NARROW_DH = 192                                          # dh <= 192: k_head_rows<1,12,3>, beyond: <1,16,4> (rd_head.hip head_route)


def _c(T, B, D, Fe, ds, C, **kw):
    return dict(T=T, B=B, D=D, Fe=Fe, ds=ds, C=C, **kw)


# ---- cases: name -> (T, B, D, Fe, d_static, C) + lengths / layout / labels -----------------------------------------------------------------
# lengths: explicit, or drawn in [0, T] with lengths[0] = T and lengths[1] = 1.  Small: T = 7, B = 5 (four gaps per unit to choose from).
CASES = {
    # instantiation edge: the <1,12,3> form covers 192 x 192; 193 is the first width on the generic one; P19's width
    "DH192": _c(7, 5, 160, 32, 3, 2), "DH193": _c(7, 5, 160, 33, 3, 2), "DH186": _c(7, 5, 152, 34, 6, 2),
    # maximum width
    "DH256_F0": _c(7, 5, 256, 0, 0, 2), "DH256_F32": _c(7, 5, 224, 32, 3, 2),
    # lane slots (64 columns per lane slot) and W0 rows per wave (16 waves)
    "DH64": _c(7, 5, 64, 0, 0, 2), "DH65": _c(7, 5, 64, 1, 3, 2), "DH128": _c(7, 5, 128, 0, 0, 2), "DH129": _c(7, 5, 128, 1, 3, 2),
    "DH16": _c(7, 5, 16, 0, 0, 2), "DH17": _c(7, 5, 16, 1, 3, 2), "DH4": _c(7, 5, 4, 0, 0, 2),
    # steps: 16 time groups x 4 steps = 64 per pass of the masked mean
    "T1": _c(1, 4, 16, 4, 3, 2, lengths=(1, 0, 1, 1)), "T16": _c(16, 5, 16, 4, 3, 2, lengths=(16, 1, 15, 0, 8)),
    "T17": _c(17, 5, 16, 4, 3, 2, lengths=(17, 1, 16, 0, 9)), "T64": _c(64, 5, 16, 4, 3, 2, lengths=(64, 1, 63, 0, 33)),
    "T65": _c(65, 5, 16, 4, 3, 2, lengths=(65, 1, 64, 63, 0)), "T128": _c(128, 6, 16, 4, 3, 2, lengths=(128, 1, 63, 65, 127, 0)),
    "T129": _c(129, 7, 16, 4, 3, 2, lengths=(129, 1, 63, 65, 127, 128, 0)), "T600": _c(600, 3, 16, 4, 3, 2, lengths=(600, 65, 0)),
    # batch: k_head_wgrad stages 256 rows per chunk
    "B1": _c(3, 1, 16, 4, 3, 2, lengths=(2,)), "B255": _c(3, 255, 16, 4, 3, 2), "B256": _c(3, 256, 16, 4, 3, 2),
    "B257": _c(3, 257, 16, 4, 3, 2), "B513": _c(3, 513, 16, 4, 3, 2),
    # classes; C dh around the 1024 threads that fetch w2 in one go
    "C1": _c(7, 5, 16, 4, 3, 1), "C2": _c(7, 5, 16, 4, 3, 2), "C16": _c(7, 5, 16, 4, 3, 16),
    "C4_DH256": _c(7, 5, 256, 0, 0, 4), "C5_DH205": _c(7, 5, 204, 1, 3, 5), "C16_DH256": _c(7, 5, 256, 0, 0, 16),
    # static embedding: in LDS where Fe ds <= 1024 and ds <= 64, else read in place; k-tiles and n-tiles of its weight-gradient job
    "EMB_32x32": _c(7, 5, 16, 32, 32, 2), "EMB_33x32": _c(7, 5, 16, 33, 32, 2), "EMB_DS64": _c(7, 5, 16, 16, 64, 2),
    "EMB_DS65": _c(7, 5, 16, 4, 65, 2), "EMB_DS17": _c(7, 5, 16, 4, 17, 2), "FE16": _c(7, 5, 16, 16, 3, 2), "FE17": _c(7, 5, 16, 17, 3, 2),
    # token plan
    "PLAN_TIES": _c(12, 7, 16, 4, 3, 2, lengths=(5, 9, 5, 1, 9, 7, 5), layout="plan"),
    "PLAN_ZEROS": _c(12, 8, 16, 4, 3, 2, lengths=(4, 0, 6, 0, 3, 12, 0, 0), layout="plan"),
    "PLAN_SINGLE": _c(12, 1, 16, 4, 3, 2, lengths=(7,), layout="plan"),
    "PLAN_ONES": _c(12, 5, 16, 4, 3, 2, lengths=(1, 1, 1, 1, 1), layout="plan"),
    "PLAN_T65": _c(65, 6, 16, 4, 3, 2, lengths=(65, 1, 64, 63, 0, 65), layout="plan"),
    "PLAN_T129": _c(129, 8, 16, 4, 3, 2, lengths=(129, 1, 63, 65, 127, 128, 0, 129), layout="plan"),
    "PLAN_DH186": _c(7, 5, 152, 34, 6, 2, lengths=(3, 7, 0, 7, 1), layout="plan"),
    "PLAN_DH193": _c(7, 5, 160, 33, 3, 2, lengths=(3, 7, 0, 7, 1), layout="plan"),
    "PLAN_DH256": _c(7, 5, 256, 0, 0, 2, lengths=(3, 7, 0, 7, 1), layout="plan"),
    # the criterion: the label count loop (1024 labels per pass), a class nobody carries, a class of weight 0
    "CRIT_B1024": _c(1, 1024, 4, 0, 0, 3), "CRIT_B1025": _c(1, 1025, 4, 0, 0, 3),
    "CRIT_ABSENT": _c(7, 5, 16, 4, 3, 4, labels=(0, 1, 3)), "CRIT_W0": _c(7, 5, 16, 4, 3, 3, zero_weight=1),
}
GROUPS = {
    "instantiation": ("DH192", "DH193", "DH186"),
    "max_width": ("DH256_F0", "DH256_F32"),
    "lane_slots": ("DH64", "DH65", "DH128", "DH129", "DH16", "DH17", "DH4"),
    "steps": ("T1", "T16", "T17", "T64", "T65", "T128", "T129", "T600"),
    "batch": ("B1", "B255", "B256", "B257", "B513"),
    "classes": ("C1", "C2", "C16", "C4_DH256", "C5_DH205", "C16_DH256"),
    "static_embedding": ("EMB_32x32", "EMB_33x32", "EMB_DS64", "EMB_DS65", "EMB_DS17", "FE16", "FE17"),
    "token_plan": ("PLAN_TIES", "PLAN_ZEROS", "PLAN_SINGLE", "PLAN_ONES", "PLAN_T65", "PLAN_T129", "PLAN_DH186", "PLAN_DH193", "PLAN_DH256"),
    "criterion": ("CRIT_B1024", "CRIT_B1025", "CRIT_ABSENT", "CRIT_W0"),
}
GROUP_OF = {n: g for g, names in GROUPS.items() for n in names}
ALL_CASES = tuple(n for names in GROUPS.values() for n in names)
assert sorted(ALL_CASES) == sorted(CASES)
FE0_CASES = tuple(n for n in ALL_CASES if CASES[n]["Fe"] == 0)          # the "Fe = 0" entry of the static-embedding list
# every case runs the plain head; these run the criterion too (eps = EPS, random positive weights) / rd_head_backward under a random cotangent
CRIT_CASES = GROUPS["criterion"] + ("DH186", "DH193", "DH256_F32", "T65", "B257", "C1", "C16", "C16_DH256", "EMB_33x32", "PLAN_TIES",
                                    "PLAN_ZEROS", "PLAN_DH186", "PLAN_DH256")
COT_CASES = ("DH192", "DH193", "DH256_F32", "DH4", "T129", "B1", "B257", "C16_DH256", "EMB_DS65", "EMB_DS17", "PLAN_TIES", "PLAN_ZEROS",
             "PLAN_T65", "PLAN_DH193")
RUNS = tuple((n, "plain") for n in ALL_CASES) + tuple((n, "crit") for n in CRIT_CASES) + tuple((n, "cot") for n in COT_CASES)
PRECISION_CASE, DEFER_CASE, ORDER_CASES = "DH193", "DH186", ("DH186", "B257", "PLAN_TIES")

# A case whose gap-placed biases miss GATE_MARGIN gets another seed here -- never another margin.
SEED_BUMP = {}

# wrong kernel -> (case the table names for that branch, loss form): each must miss a working bound by more than 10 x
VARIANTS = {
    "len_div": ("DH17", "plain"),             # the mean divided by len, not len + 1
    "drop_t64": ("T65", "plain"),             # the masked mean's later passes (steps >= 64) never run
    "one_past": ("T17", "plain"),             # one step past the length read
    "feat_cols192": ("DH193", "plain"),       # feature columns >= 192 dropped from w0 feat
    "hid_rows192": ("DH193", "plain"),        # hidden rows >= 192 dropped
    "wgrad_b256": ("B257", "plain"),          # rows b >= 256 dropped from the weight gradients
    "embw_ds16": ("EMB_DS17", "plain"),       # d_static columns >= 16 dropped from d emb_w
    "w2_1024": ("C5_DH205", "plain"),         # w2 elements >= 1024 never reach LDS
    "no_emb_b": ("FE16", "plain"),            # emb_b omitted
    "crit_norm_B": ("CRIT_W0", "crit"),       # the weighted loss normalised by B, not W
    "count_1024": ("CRIT_B1025", "crit"),     # only the first 1024 labels counted into W
    "dr_pad": ("T16", "plain"),               # dr at a padded step not zero
    "tie_swap": ("PLAN_TIES", "plain"),       # the plan rows of two samples of equal length exchanged
}


def dh_of(c):
    return c["D"] + c["Fe"]


def instantiation(c, crit):
    """the launch-log name of the case's k_head_rows (RD_HEAD_NARROW at its default)"""
    return "k_head_rows<%s%s>" % ("12,3" if dh_of(c) <= NARROW_DH else "16,4", ",crit" if crit else "")


def _rng(*key):
    return np.random.default_rng([zlib.crc32(repr(key).encode()), SEED_BUMP.get(key[0], 0)])


def _mm(a, b):
    """[M, N] = sum_k a[m, k] b[n, k], a running sum over k in the operands' precision"""
    out = np.zeros((a.shape[0], b.shape[0]), dtype=a.dtype)
    for k in range(a.shape[1]):
        out = out + a[:, k:k + 1] * b[None, :, k]
    return out


def _seq_sum(a, axis=0):
    a = np.moveaxis(a, axis, 0)
    s = np.zeros(a.shape[1:], dtype=a.dtype)
    for i in range(a.shape[0]):
        s = s + a[i]
    return s


def keep_of(lengths, T):
    """[T, B] bool: the live steps (the complement of the padding mask)"""
    return np.arange(T)[:, None] < np.asarray(lengths)[None, :]


def rows_of(c, full):
    """[T, B, D] -> [M_live, D] in plan order (tests/helpers.plan_ref)"""
    p = plan_ref(c["lengths"], c["T"])
    out = np.zeros((p["mlive"], full.shape[2]), dtype=full.dtype)
    for r, b in enumerate(p["order"]):
        out[p["off"][r]:p["off"][r + 1]] = full[:p["lenr"][r], b]
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs of one case (fp32 / int64 arrays; treat as read-only)"""
    t = CASES[name]
    T, B, D, Fe, ds, C = (t[k] for k in ("T", "B", "D", "Fe", "ds", "C"))
    dh = D + Fe
    rng = _rng(name, T, B, D, Fe, ds, C)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    if "lengths" in t:
        lengths = np.array(t["lengths"], dtype=np.int64)
    else:
        lengths = rng.integers(0, T + 1, size=B).astype(np.int64)
        lengths[0] = T
        if B > 1:
            lengths[1] = 1
    assert lengths.shape == (B,) and lengths.min() >= 0 and lengths.max() <= T
    c = dict(name=name, group=GROUP_OF[name], T=T, B=B, D=D, Fe=Fe, ds=ds, C=C, dh=dh, layout=t.get("layout", "padded"), lengths=lengths)
    c["r"] = f32(rng.standard_normal((T, B, D)) + rng.standard_normal((1, B, D)))       # a per-sample offset: agg is O(1) at any length
    c["stat"] = f32(rng.standard_normal((B, ds)))
    c["emb_w"] = f32(rng.standard_normal((Fe, ds)) / np.sqrt(max(ds, 1)))
    c["emb_b"] = f32(0.3 * rng.standard_normal(Fe))
    c["w0"] = f32(rng.standard_normal((dh, dh)) / np.sqrt(dh))
    c["w2"] = f32(rng.standard_normal((C, dh)) * (2.0 / np.sqrt(dh)))
    c["b2"] = f32(0.1 * rng.standard_normal(C))
    labels = np.array(t.get("labels", tuple(range(C))), dtype=np.int64)
    c["y"] = labels[rng.integers(0, len(labels), size=B)]
    if len(labels) > 1 and B >= len(labels):
        c["y"][:len(labels)] = labels                                                    # every listed class is present
    w = rng.uniform(0.5, 1.5, size=C)
    if "zero_weight" in t:
        w[t["zero_weight"]] = 0.0
    c["crit"] = f32(np.concatenate([[EPS], w]))
    c["dlog_in"] = f32(rng.standard_normal((B, C)) / B)
    # decisive gates
    c["b0"] = np.zeros(dh, dtype=np.float32)
    z = evaluate(c, "plain")["pre"]                                                      # w0 feat in float64 (b0 = 0)
    if B == 1:
        b0 = -z[0] + B1_OFFSET * np.where(np.arange(dh) % 2 == 0, 1.0, -1.0)
    else:
        s = np.sort(z, axis=0)
        i = np.argmax(s[1:] - s[:-1], axis=0)
        b0 = -0.5 * (s[i, np.arange(dh)] + s[i + 1, np.arange(dh)])
    c["b0"] = f32(b0)
    return c


# ---- the reference --------------------------------------------------------------------------------------------------------------------------
def evaluate(c, form="plain", dtype=np.float64, variant=None, dlog_in=None):
    """{loss, logits, pre, dlog, dr, dW0, db0, dW2, db2, demb_w, demb_b} of case c in `dtype` (float64: the reference; float32: the
    yardstick).  form: one of FORMS; dlog_in: the cotangent of "cot" (default the case's).  variant: one of VARIANTS -- a WRONG kernel,
    for tests/test_head_ref_host.py.  dr: [T, B, D], or [M_live, D] on the plan layout."""
    f = dtype
    T, B, D, Fe, C, dh = c["T"], c["B"], c["D"], c["Fe"], c["C"], c["dh"]
    lengths = c["lengths"]
    r, stat, emb_w, emb_b = c["r"].astype(f), c["stat"].astype(f), c["emb_w"].astype(f), c["emb_b"].astype(f)
    w0, b0, w2, b2, y = c["w0"].astype(f), c["b0"].astype(f), c["w2"].astype(f), c["b2"].astype(f), c["y"]
    if variant == "tie_swap":
        b1, b2_ = next((i, j) for i in range(B) for j in range(i + 1, B) if lengths[i] == lengths[j] and lengths[i] > 0)
        r = r.copy()
        r[:, [b1, b2_]] = r[:, [b2_, b1]]
    if variant == "w2_1024":
        w2 = w2.copy()
        w2.reshape(-1)[1024:] = 0
    if variant == "no_emb_b":
        emb_b = np.zeros_like(emb_b)
    keep = keep_of(lengths, T)
    fkeep = keep
    if variant == "drop_t64":
        fkeep = keep & (np.arange(T) < 64)[:, None]
    if variant == "one_past":
        fkeep = np.arange(T)[:, None] <= lengths[None, :]
    den = np.maximum(lengths, 1) if variant == "len_div" else lengths + 1
    il = f(1.0) / den.astype(f)                                                          # [B]
    agg = _seq_sum(r * fkeep[:, :, None].astype(f)) * il[:, None]
    feat = np.concatenate([agg, _mm(stat, emb_w) + emb_b[None, :]], axis=1) if Fe else agg
    featp = feat
    if variant == "feat_cols192":
        featp = feat.copy()
        featp[:, 192:] = 0
    pre = _mm(featp, w0) + b0[None, :]
    hid = np.maximum(pre, f(0.0))
    if variant == "hid_rows192":
        hid = hid.copy()
        hid[:, 192:] = 0
    logits = _mm(hid, w2) + b2[None, :]
    res = dict(logits=logits, pre=pre, loss=None)
    # ---- the loss and d loss / d logits ----
    m = logits.max(1, keepdims=True)
    lse = m + np.log(_seq_sum(np.exp(logits - m), 1))[:, None]
    p = np.exp(logits - lse)
    onehot = (np.arange(C)[None, :] == y[:, None]).astype(f)
    nll = (lse - logits)[np.arange(B), y]
    if form == "plain":
        res["loss"] = _seq_sum(nll) / f(B)
        dlog = (p - onehot) * (f(1.0) / f(B))
    elif form == "crit":
        eps, w = c["crit"][0].astype(f), c["crit"][1:].astype(f)
        counted = y[:1024] if variant == "count_1024" else y
        n = np.bincount(counted, minlength=C).astype(f)
        W = f(B) if variant == "crit_norm_B" else _seq_sum(n * w)
        wy, sw = w[y], _seq_sum(w)
        sm = _seq_sum((lse - logits) * w[None, :], 1)
        term = (f(1.0) - eps) * wy * nll + (eps / f(C)) * sm
        res["loss"] = _seq_sum(term) / W
        dlog = ((f(1.0) - eps) * (p - onehot) * (wy / W)[:, None] + (eps / f(C) / W) * (p * sw - w[None, :])).astype(f)
    else:
        dlog = (c["dlog_in"] if dlog_in is None else dlog_in).astype(f)
    res["dlog"] = dlog
    # ---- backward ----
    dhid = _mm(dlog, w2.T) * (pre > 0).astype(f)
    dfeat = _mm(dhid, w0.T)
    nb = 256 if variant == "wgrad_b256" else B                                           # rows that reach the weight gradients
    res["dW2"], res["db2"] = _mm(dlog[:nb].T, hid[:nb].T), _seq_sum(dlog[:nb])
    res["dW0"], res["db0"] = _mm(dhid[:nb].T, feat[:nb].T), _seq_sum(dhid[:nb])
    demb = dfeat[:, D:]
    res["demb_w"], res["demb_b"] = _mm(demb[:nb].T, stat[:nb].T), _seq_sum(demb[:nb])
    if variant == "embw_ds16":
        res["demb_w"] = res["demb_w"].copy()
        res["demb_w"][:, 16:] = 0
    bkeep = np.ones_like(keep) if variant == "dr_pad" else keep
    dr = bkeep[:, :, None].astype(f) * (dfeat[:, :D] * il[:, None])[None, :, :]
    res["dr"] = rows_of(c, dr) if c["layout"] == "plan" else dr
    return res


_REF = {}


def reference(name, form, dtype=np.float64):
    """evaluate() of a case, computed once per (case, form, precision) and shared: callers must not modify it"""
    key = (name, form, np.dtype(dtype).name)
    if key not in _REF:
        _REF[key] = evaluate(case(name), form, dtype)
    return _REF[key]


def gate_margin(name):
    """smallest |pre-activation| of the case in float64 under its fp32 b0"""
    return float(np.abs(reference(name, "plain")["pre"]).min())


# ---- errors and bounds ----------------------------------------------------------------------------------------------------------------------
def _norm(tensor, ref):
    ref = np.asarray(ref, dtype=np.float64)
    n = float(np.abs(ref).max()) if ref.size else 0.0
    return max(1.0, n) if tensor == "loss" else n


def error_of(tensor, got, ref):
    """max |got - ref| over the reference's max-norm (the loss: over max(1, |ref|)); where the norm is 0, 0 or inf"""
    a, r = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == r.shape, (tensor, a.shape, r.shape)
    if a.size == 0:
        return 0.0
    if not np.isfinite(a).all():
        return np.inf
    e, n = float(np.abs(a - r).max()), _norm(tensor, r)
    return e / n if n > 0 else (0.0 if e == 0 else np.inf)


def floor_of(tensor, ref):
    """8 fp32 ulps of the tensor's max-norm, relative to it"""
    n = _norm(tensor, ref)
    return FLOOR_ULPS * float(np.spacing(np.float32(n))) / n if n > 0 else 0.0


def tensors_of(form):
    """what a run of the form returns: rd_head_backward ("cot") has neither a loss nor logits"""
    return GRADS if form == "cot" else ("loss",) + COMPARED


def yardstick(name, form, tensor):
    """the float32 evaluation's error against the float64 one, not below the floor"""
    r64, r32 = reference(name, form), reference(name, form, np.float32)
    return max(error_of(tensor, r32[tensor], r64[tensor]), floor_of(tensor, r64[tensor]))


def bound_of(name, form, tensor):
    """working bound: min(ceiling, 4 x yardstick).  Takes the ceilings and the CPU yardstick only."""
    return min(LOSS_CEILING if tensor == "loss" else CEILING, YARD_FACTOR * yardstick(name, form, tensor))


def compare(name, form, got, ref=None):
    """[(tensor, error, bound, yardstick)] of every compared tensor of a run, and the tensors that are not exactly zero where the
    float64 reference is"""
    ref = reference(name, form) if ref is None else ref
    rows, nonzero = [], []
    for t in tensors_of(form):
        rows.append((t, error_of(t, got[t], ref[t]), bound_of(name, form, t), yardstick(name, form, t)))
        if (np.asarray(got[t])[np.asarray(ref[t]) == 0] != 0).any():
            nonzero.append(t)
    return rows, nonzero


def variant_margin(variant):
    """largest error / working bound over the compared tensors of the wrong kernel `variant` (inf where an exact zero is missed)"""
    name, form = VARIANTS[variant]
    rows, nonzero = compare(name, form, evaluate(case(name), form, variant=variant))
    if nonzero:
        return np.inf
    return max((e / b if b > 0 else (np.inf if e > 0 else 0.0)) for _, e, b, _ in rows)
