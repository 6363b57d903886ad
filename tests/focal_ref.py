"""TEST INFRASTRUCTURE ONLY -- the focal loss of the fused head and the captured steps (rd_softmax_xent_focal, rd_head_train_focal:
k_softmax_xent_focal, k_head_rows<.,.,focal>): float64 reference, inputs and bounds.

Used by tests/test_focal_ref_host.py (conditions on the reference alone, no GPU) and tests/test_focal_gpu.py.

Reference (numpy; `loss_and_dlogits`).  For logits z [B, C], labels y, class weights w >= 0 and gamma >= 0:
    p       = softmax(z),  logp_y = z[b, y_b] - lse_b
    q_b     = sum over c != y_b, ascending, of p[b, c]                (not 1 - p_y)
    m_b     = q_b^gamma                                               (gamma == 0: 1;  q_b == 0 and gamma > 0: 0)
    g_b     = m_b - gamma p_y q_b^(gamma - 1) logp_y                  (gamma == 0: 1;  q_b == 0 and gamma > 0: 0;  the second term
                                                                       is 0 wherever logp_y has rounded to 0: its limit, never 0 * inf)
    W       = sum over c ascending of n_c w_c                         (n_c: labels equal to c)
    loss    = sum_b w[y_b] m_b (-logp_y) / W
    dlogits = (p - onehot) g_b w[y_b] / W
`evaluate` puts the whole head under it on tests/head_ref.py's cases: head_ref's forward pieces give the logits, the formulas above the
loss and d loss / d logits, and head_ref's hand-written backward (its "cot" form) every gradient.  All of it runs in the dtype asked
for, running sums included, so the same code in float32 is the yardstick.

Bounds: the project's rule (tests/head_ref.py `bound_of`): min(ceiling, 4 x the float32 evaluation's error against the float64 one,
the yardstick never below 8 fp32 ulps of the tensor's max-norm); ceilings 1e-6 on the loss relative to max(1, |loss|) and 2e-5 of the
float64 max-norm on everything else.  No bound reads a device number."""
import functools
import zlib

import numpy as np

from tests import head_ref as HR

GAMMAS = (0.0, 0.5, 1.0, 2.0, 5.0)
SMALL_GAMMAS = (0.05, 0.1)                               # with a logit gap near 100: q^(gamma - 1) overflows fp32 while q is a positive denormal
OP_B, OP_C = (1, 3, 64, 1025), (1, 2, 8, 16, 17)
OP_TENSORS = ("loss", "dlogits")
VARIANTS = ("g_first_term_only", "denominator_B", "q_one_minus_py_f32", "gamma_on_py")

# two more cases for the fused head beside head_ref's table, kept HERE (`case`): B = 3, T = 5; and the same shape with b2 = [+100, 0],
# which puts a logit gap near 100 under every sample -- confidently right for label 0, confidently wrong for label 1
LOCAL_CASES = {"FOCAL_B3_T5": dict(T=5, B=3, D=16, Fe=4, ds=3, C=2, lengths=(5, 0, 2), y=(0, 1, 0), b2=(0.1, -0.05)),
               "FOCAL_GAP100": dict(T=5, B=3, D=16, Fe=4, ds=3, C=2, lengths=(5, 2, 0), y=(0, 1, 0), b2=(100.0, 0.0))}
# (there the confidently wrong sample has live steps: dr is then of ordinary size.  Were the confident samples the only ones with rows,
# dr would be ~1e-45 throughout, below what fp32 holds at all)
# (case, gamma): the narrow form at P19's width and at dh = 192, the wide form at dh = 193 and 256; B = 1, 3, 257 (k_head_wgrad's chunk
# edge) and 1025 (the label count's second pass); T = 1, 5, 65; C = 2 and 16; with and without the static embedding; padded layout
# and token plan (with zero lengths); an absent class and a class of weight zero
HEAD_RUNS = (("DH186", 2.0), ("DH192", 0.5), ("DH193", 2.0), ("PLAN_DH186", 2.0), ("PLAN_DH193", 0.5), ("PLAN_ZEROS", 1.0), ("B1", 2.0),
             ("FOCAL_B3_T5", 1.0), ("B257", 2.0), ("T1", 5.0), ("T65", 2.0), ("C16", 2.0), ("C16_DH256", 0.5), ("DH256_F0", 2.0), ("DH64", 1.0),
             ("CRIT_B1025", 2.0), ("CRIT_W0", 2.0), ("CRIT_ABSENT", 0.5), ("FOCAL_GAP100", 0.05), ("FOCAL_GAP100", 0.1), ("FOCAL_GAP100", 2.0))
HEAD_ZERO_RUNS = ("DH186", "DH193", "PLAN_ZEROS", "B257", "C16", "CRIT_B1025")          # gamma = 0 against rd_head_train_crit at eps = 0


def instantiation(c):
    return "k_head_rows<%s,focal>" % ("12,3" if HR.dh_of(c) <= HR.NARROW_DH else "16,4")


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs of one case, in head_ref.case's form (treat as read-only): head_ref's own for its names, LOCAL_CASES built here by
    head_ref's rules -- b0[j] is minus the midpoint of the widest gap between the sorted float64 pre-activations of unit j"""
    if name not in LOCAL_CASES:
        return HR.case(name)
    t = LOCAL_CASES[name]
    T, B, D, Fe, ds, C = (t[k] for k in ("T", "B", "D", "Fe", "ds", "C"))
    dh = D + Fe
    rng = np.random.default_rng([zlib.crc32(b"focal_head"), T, B, D, Fe, ds, C])
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    c = dict(name=name, group="focal", T=T, B=B, D=D, Fe=Fe, ds=ds, C=C, dh=dh, layout="padded", lengths=np.array(t["lengths"], dtype=np.int64))
    c["r"] = f32(rng.standard_normal((T, B, D)) + rng.standard_normal((1, B, D)))
    c["stat"] = f32(rng.standard_normal((B, ds)))
    c["emb_w"] = f32(rng.standard_normal((Fe, ds)) / np.sqrt(ds))
    c["emb_b"] = f32(0.3 * rng.standard_normal(Fe))
    c["w0"] = f32(rng.standard_normal((dh, dh)) / np.sqrt(dh))
    c["w2"] = f32(rng.standard_normal((C, dh)) * (2.0 / np.sqrt(dh)))
    c["b2"] = f32(t["b2"])
    c["y"] = np.array(t["y"], dtype=np.int64)
    c["crit"] = f32(np.concatenate([[HR.EPS], rng.uniform(0.5, 1.5, size=C)]))
    c["dlog_in"] = f32(np.zeros((B, C)))
    c["b0"] = np.zeros(dh, dtype=np.float32)
    s = np.sort(HR.evaluate(c, "cot")["pre"], axis=0)                  # w0 feat in float64 (b0 = 0)
    i = np.argmax(s[1:] - s[:-1], axis=0)
    c["b0"] = f32(-0.5 * (s[i, np.arange(dh)] + s[i + 1, np.arange(dh)]))
    return c


def gate_margin(name):
    """smallest |pre-activation| of the case in float64 under its fp32 b0"""
    return float(np.abs(HR.evaluate(case(name), "cot")["pre"]).min())


# ---- the loss ---------------------------------------------------------------------------------------------------------------------------------
def loss_and_dlogits(logits, y, w, gamma, dtype=np.float64, variant=None):
    """(loss, dlogits [B, C]) in `dtype`; variant: one of VARIANTS -- a WRONG kernel, for tests/test_focal_ref_host.py"""
    f = dtype
    z, w, gamma = np.asarray(logits).astype(f), np.asarray(w).astype(f), f(gamma)
    B, C = z.shape
    m_ = z.max(1, keepdims=True)
    lse = m_ + np.log(HR._seq_sum(np.exp(z - m_), 1))[:, None]
    p = np.exp(z - lse)
    hot = np.arange(C)[None, :] == np.asarray(y)[:, None]
    nll = (lse - z)[np.arange(B), y]
    py = p[np.arange(B), y]
    q = HR._seq_sum(np.where(hot, f(0), p), 1)
    if variant == "q_one_minus_py_f32":
        q = (np.float32(1.0) - py.astype(np.float32)).astype(f)
    base = py if variant == "gamma_on_py" else q
    live = base > 0
    safe = np.where(live, base, f(1))
    if gamma == 0:
        m, g = np.ones(B, dtype=f), np.ones(B, dtype=f)
    else:
        m = np.where(live, np.exp(gamma * np.log(safe)), f(0)).astype(f)
        with np.errstate(over="ignore", invalid="ignore"):
            second = np.where(nll == 0, f(0), gamma * py * np.exp((gamma - f(1)) * np.log(safe)) * nll)
        g = np.where(live, m + second, f(0)).astype(f)
        if variant == "g_first_term_only":
            g = m
    n = np.bincount(y, minlength=C).astype(f)
    W = f(B) if variant == "denominator_B" else HR._seq_sum(n * w)
    wy = w[y]
    with np.errstate(divide="ignore", invalid="ignore"):
        loss = HR._seq_sum(wy * m * nll) / W
        dlog = ((p - hot.astype(f)) * g[:, None] * (wy / W)[:, None]).astype(f)
    return f(loss), dlog


# ---- operator inputs -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def op_case(B, C):
    """logits [B, C] fp32, y [B], w [C] fp32 of the stand-alone operator's case.  Rows by b mod 6: random; confidently right (logit gap
    130: the other classes' fp32 probabilities are exactly 0); confidently wrong; an exact tie of all classes; moderately confident;
    random.  With C >= 3 the last class is absent from the labels; with C >= 2 class 1 has weight zero; sample 0 carries class 0, whose
    weight is positive, so W > 0."""
    rng = np.random.default_rng([zlib.crc32(b"focal_op"), B, C])
    allowed = np.arange(C - 1 if C >= 3 else C)
    y = allowed[rng.integers(0, len(allowed), size=B)].astype(np.int64)
    y[0] = 0
    z = 2.0 * rng.standard_normal((B, C))
    for b in range(B):
        other = (y[b] + 1) % C
        k = b % 6
        if k == 1:
            z[b] = -60.0 - rng.uniform(0, 3, size=C); z[b, y[b]] = 70.0
        elif k == 2 and C > 1:
            z[b] = rng.standard_normal(C); z[b, y[b]] = -60.0; z[b, other] = 70.0
        elif k == 3:
            z[b] = 0.25
        elif k == 4:
            z[b, y[b]] += 10.0
    w = rng.uniform(0.5, 1.5, size=C)
    if C >= 2:
        w[1] = 0.0
    return dict(B=B, C=C, logits=np.ascontiguousarray(z, dtype=np.float32), y=y, w=np.ascontiguousarray(w, dtype=np.float32),
                confident=np.array([b for b in range(B) if b % 6 == 1], dtype=np.int64))


@functools.lru_cache(maxsize=None)
def small_gamma_case():
    """the operator at SMALL_GAMMAS: logit gaps of 90 .. 103 (fp32: q a positive denormal, lse - z_y exactly 0, q^(gamma - 1) beyond the
    largest float) on confidently right rows, the same gaps confidently wrong, and ordinary rows between them"""
    z = np.array([[100.0, 0.0, -3.0], [0.3, 0.1, -0.2], [-2.0, 101.5, 0.0], [0.0, 90.0, -1.0], [1.0, -1.0, 0.5], [103.0, 0.0, 0.0],
                  [0.0, 0.5, 97.0]], dtype=np.float32)
    y = np.array([0, 1, 1, 0, 2, 0, 2], dtype=np.int64)
    return dict(B=7, C=3, logits=z, y=y, w=np.array([1.0, 0.5, 1.5], dtype=np.float32), confident=np.array([0, 2, 5, 6], dtype=np.int64))


_OP_REF = {}


def op_reference(B, C, gamma, dtype=np.float64):
    key = (B, C, float(gamma), np.dtype(dtype).name)
    if key not in _OP_REF:
        c = op_case(B, C)
        loss, dlog = loss_and_dlogits(c["logits"], c["y"], c["w"], gamma, dtype)
        _OP_REF[key] = dict(loss=loss, dlogits=dlog)
    return _OP_REF[key]


def _bound(tensor, r32, r64):
    yard = max(HR.error_of(tensor, r32, r64), HR.floor_of(tensor, r64))
    return min(HR.LOSS_CEILING if tensor == "loss" else HR.CEILING, HR.YARD_FACTOR * yard), yard


def op_compare(got, ref64, ref32):
    """[(tensor, error, bound, yardstick)] of an operator result {loss, dlogits} against the float64 reference"""
    return [(t, HR.error_of(t, got[t], ref64[t])) + _bound(t, ref32[t], ref64[t]) for t in OP_TENSORS]


# ---- the whole head --------------------------------------------------------------------------------------------------------------------------
def head_weights(c):
    """the case's class weights (head_ref draws them for its criterion form; slot 0 there is the smoothing)"""
    return c["crit"][1:]


def focal_buffer(c, gamma):
    return np.concatenate([[np.float32(gamma)], head_weights(c)]).astype(np.float32)


def evaluate(c, gamma, dtype=np.float64, variant=None):
    """head_ref.evaluate's result dict (loss, logits, dlog, dr, dW0 .. demb_b) of case c under the focal loss, in `dtype`"""
    logits = HR.evaluate(c, "cot", dtype, dlog_in=np.zeros((c["B"], c["C"])))["logits"]
    loss, dlog = loss_and_dlogits(logits, c["y"], head_weights(c), gamma, dtype, variant)
    res = HR.evaluate(c, "cot", dtype, dlog_in=dlog)
    res["loss"] = loss
    return res


_REF = {}


def reference(name, gamma, dtype=np.float64):
    key = (name, float(gamma), np.dtype(dtype).name)
    if key not in _REF:
        _REF[key] = evaluate(case(name), gamma, dtype)
    return _REF[key]


def compare(name, gamma, got, tensors=("loss",) + HR.COMPARED):
    """[(tensor, error, bound, yardstick)] of a fused-head run, and the tensors that are not exactly zero where the reference is"""
    r64, r32 = reference(name, gamma), reference(name, gamma, np.float32)
    rows, nonzero = [], []
    for t in tensors:
        rows.append((t, HR.error_of(t, got[t], r64[t])) + _bound(t, r32[t], r64[t]))
        if (np.asarray(got[t])[np.asarray(r64[t]) == 0] != 0).any():
            nonzero.append(t)
    return rows, nonzero
