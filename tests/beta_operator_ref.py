"""TEST INFRASTRUCTURE ONLY -- the use_beta graph operator (rd_graph_beta_fwd / _bwd[_alpha | _dropout]: the LDS form of
rd_graph_beta.hip, the workspace form of rd_graph_beta_large.hip, the rounds 2-5 kernels behind RD_BETA_V1): case table, inputs,
float64 reference and bounds.

Used by tests/test_beta_operator_ref_host.py (conditions on the reference alone, no GPU) and tests/test_beta_operator_float64_gpu.py
(both forms across their envelope against this reference).

Reference (numpy; `evaluate`): code/Ob_propagation.py:161-227 on the operator's own inputs V [B,N,K], H [B,N,T,32], map_w [N,16],
p_t [B or 1,T,16], edge_index [2,E], w [B or 1,E], optionally a keep mask [B,E,T,4] and a cotangent dalpha [B,Kk]:
    beta[i,t]  = mean over the 32 channels of H[i,t,:] * cat(map_w[i], p_t[t])
    alpha[e]   = mean over t of beta[tgt(e),t] * w[e]
    kept       = the first Kk = int(E * 0.5) edges by descending alpha, ties by lower edge id, in that order
    P[q,t]     = exp(g[q,t] - max) / (sum over the kept edges of q's SOURCE + 1e-16),   g[q,t] = beta[tgt,t] * w
    out[n,4t+c] = sum over kept q with src = n of  P[q,t] * keep[e(q),t,c] / (1 - p) * V[tgt(q),4t+c]
and the chain rule written out for dV, dH, d map_w (summed over the batch), dw (exactly 0 for pruned edges) under dout and dalpha.
The mask touches the aggregation only: pruning, the lists and alpha do not see it.  `e(q)` is the INPUT edge id.
Every reduction over channels, steps and list entries is a plain running sum in the working precision (a loop over the axis;
np.add.at over the lists), so the SAME code evaluated in float32 is the yardstick: what fp32 arithmetic alone costs this operation.
tests/test_beta_operator_ref_host.py holds the float64 evaluation to torch autograd on oracle/restatement.py and to a finite difference.

Decisive pruning.  Top-K and the reordering are discontinuous, so every case keeps adjacent scores apart, per sample: the float64
scores sorted descending have (s[i] - s[i+1]) / |s[i]| >= GAP and min |s| >= GAP max |s|.  GAP >= 8 x the a-priori fp32 bound of a
score, (T + 34) 2^-24 mean|term| / |score| (32 + 2 roundings for a beta, T for the sum over steps, ~2 for the weight and the
division; a derivation, not a measurement -- `apriori_score_bound`).  Random weights cannot give this at E in the thousands, so
the weights are constructed: beta is kept positive and O(0.3); s_tgt = mean_t beta[tgt] in float64; w[e] = ladder[rank[e]] /
s_tgt(e) rounded to fp32 with ladder[r] = 2 ratio^-r, ratio = 1 + 2 GAP, and rank a seeded permutation (so pruning order, edge id,
source and target are unrelated).  GAP is raised above the minimum where E is small so that the ladder spans a factor 4 (the softmax
is not flat).  The condition is re-checked after the rounding (`conditions`); a case that misses it gets another seed through
SEED_BUMP, never a smaller margin.  Shared-weight cases at B > 1 take sample b's H as an exact power-of-two multiple of sample 0's
(and p_t, where it is per-sample, as a power-of-two multiple compensated in H's second half), with independent V.
The TIE case is separate: all scores equal and exact in fp32 and fp64 alike (H = 1, map_w = p_t = 1/4, w = 1, T = 4); it checks the
documented rule, lower edge id first, bit-exactly on the returned lists.

Bounds (`bound_of`): lists and kept ids bit-exact (what the gap buys); alpha and beta_save relative to the float64 max-norm, out
absolute, gradients relative to their float64 max-norm.  Ceilings: the project's existing figures (test_beta_operator_at_dataset_shapes,
test_values_and_gradients_against_o2_under_the_kernels_mask, the fixture test): 2e-5 on values (x 1/(1-p) under dropout), 5e-5 on
gradients, 1e-5 on alpha.  Working bound per tensor, case group and mode: min(ceiling, max(4 x yardstick, 8 x 2^-24 of the norm)),
the yardstick being the float32 evaluation's error against its float64 self, maximum over the group (`yardstick`).  bound_of takes
the ceilings and that CPU figure only: no bound reads a device number."""
import functools
import zlib

import numpy as np

from tests import rng_ref as R

D_OB = 4
P_DROP, DROP_SEED = 0.3, 20240607
MODES = ("plain", "alpha", "drop")                      # no dalpha; with dalpha; p_drop = 0.3 with dalpha
LISTS = ("ei_out", "kept")
VALUES = ("out", "alpha", "beta")
GRADS = ("dV", "dH", "dmap", "dw")
COMPARED = VALUES + GRADS
CEILING = dict(out=2e-5, beta=2e-5, alpha=1e-5, dV=5e-5, dH=5e-5, dmap=5e-5, dw=5e-5)
FLOOR = 8.0 * 2.0 ** -24
YARD_FACTOR = 4.0
LADDER_TOP, LADDER_SPAN = 2.0, 4.0

# ---- cases: name -> (N, E, T, B, graph kind, w per-sample, p_t per-sample) ------------------------------------------------------------
# Kk = int(E / 2).  LDS form: N <= 64 and E <= 4096; 16 waves build the per-node lists round-robin, 64 kept positions per ballot.
_PS = (True, True)
CASES = {
    # LDS form, list geometry: ballot tails (Kk around 64 and 128), node counts around the 16 waves
    "KK63": (20, 126, 8, 2, "rand") + _PS, "KK64": (20, 129, 8, 2, "rand") + _PS, "KK65": (20, 130, 6, 2, "rand") + _PS,
    "KK129": (24, 258, 5, 2, "rand") + _PS,
    "N1": (1, 10, 4, 2, "rand") + _PS, "N2": (2, 12, 4, 2, "rand") + _PS, "N15": (15, 90, 7, 2, "rand") + _PS,
    "N16": (16, 100, 9, 2, "rand") + _PS, "N17": (17, 110, 16, 2, "rand") + _PS, "N33": (33, 200, 5, 2, "rand") + _PS,
    "N64": (64, 300, 12, 2, "rand") + _PS,
    "NOOUT": (18, 120, 6, 2, "no_out") + _PS,          # a third of the nodes own no out-edge; node 0 has in-edges only, all pruned
    "SELF": (12, 40, 5, 2, "self") + _PS,              # self-loops only
    "DUP": (10, 80, 6, 2, "dup") + _PS,                # every edge twice
    "ONESRC": (9, 50, 7, 2, "one_src") + _PS, "ONETGT": (9, 50, 7, 2, "one_tgt") + _PS,
    # LDS form, degenerate edge counts (Kk = 0, 0, 1, 1)
    "E0": (5, 0, 4, 2, "rand") + _PS, "E1": (5, 1, 4, 2, "rand") + _PS, "E2": (5, 2, 4, 2, "rand") + _PS, "E3": (5, 3, 4, 2, "rand") + _PS,
    # LDS form, capacity edges: STAGE_V true / false; backward chunks Tc < T with T % Tc != 0 (Tc depends on dalpha and dropout)
    "CAP_T48": (64, 4096, 48, 2, "rand") + _PS, "CAP_T64": (64, 4096, 64, 2, "rand") + _PS,
    "CAP_T7": (64, 4096, 7, 2, "rand") + _PS, "CAP_T5": (64, 4096, 5, 2, "rand") + _PS,
    "P19": (34, 578, 60, 2, "rand") + _PS,             # the P19 shape with 34 x 17 edges (the step benchmark's edge count)
    "CAP_T125": (64, 300, 125, 2, "rand") + _PS,       # the rounds 2-5 backward halves its chunk: 63 + 62 steps (round 6: 42 + 42 + 41)
    # hand-over between the forms
    "H_E4097": (64, 4097, 4, 2, "rand") + _PS, "H_N65": (65, 200, 4, 2, "rand") + _PS,
    # workspace form: P2 = 8192, 16384 (global merge stages, pad keys in more than one 4096-key chunk), Kk > 8192, the node limit
    "W_E8193": (40, 8193, 4, 2, "rand") + _PS, "W_E12289": (40, 12289, 4, 2, "rand") + _PS,
    "W_KK8200": (129, 16400, 4, 2, "rand") + _PS, "W_N1024": (1024, 3000, 4, 2, "rand") + _PS,
    # strides at B = 3: (w per-sample, p_t per-sample)
    "S_WS_PP": (12, 60, 6, 3, "rand", False, True), "S_WP_PS": (12, 60, 6, 3, "rand", True, False),
    "S_WP_PP": (12, 60, 6, 3, "rand", True, True), "S_WS_PS": (12, 60, 6, 3, "rand", False, False),
    # all scores equal: the tie rule
    "TIE": (8, 20, 4, 2, "tie", False, False),
}
GROUPS = {
    "lds_geometry": ("KK63", "KK64", "KK65", "KK129", "N1", "N2", "N15", "N16", "N17", "N33", "N64", "NOOUT", "SELF", "DUP",
                     "ONESRC", "ONETGT"),
    "lds_degenerate": ("E0", "E1", "E2", "E3"),
    "lds_capacity": ("CAP_T48", "CAP_T64", "CAP_T7", "CAP_T5", "P19", "CAP_T125"),
    "handover": ("H_E4097", "H_N65"),
    "workspace": ("W_E8193", "W_E12289", "W_KK8200", "W_N1024"),
    "strides": ("S_WS_PP", "S_WP_PS", "S_WP_PP", "S_WS_PS"),
    "tie": ("TIE",),
}
GROUP_OF = {n: g for g, names in GROUPS.items() for n in names}
ALL_CASES = tuple(n for names in GROUPS.values() for n in names)
assert sorted(ALL_CASES) == sorted(CASES)
LDS_CASES = GROUPS["lds_geometry"] + GROUPS["lds_degenerate"] + GROUPS["lds_capacity"] + GROUPS["strides"] + GROUPS["tie"]
WORKSPACE_CASES = GROUPS["handover"] + GROUPS["workspace"]
FORCED_LARGE = ("KK65", "NOOUT", "N17")                 # LDS list-geometry cases again under RD_BETA_LARGE=1
V1_CASES = ("KK65", "N17", "NOOUT", "E1", "E3", "CAP_T7", "CAP_T5", "CAP_T64", "CAP_T125", "S_WP_PS")    # under RD_BETA_V1=1, no dalpha
REFUSED_N = 1025
STAGE_V = {"CAP_T48": True, "CAP_T64": False}           # what the route query must report
PRECISION_CASES = ("KK65", "CAP_T7", "W_E8193")
CHUNK_CASE, CHUNK_TC = "CAP_T7", 4                      # plain backward at (64, 4096, 7): two passes of 4 + 3 steps (asserted on the route)
# steps per pass of the round 6 backward, (plain, alpha, drop): the alpha arrays and the keep-code plane each shrink the chunk.  Written
# out from lds2_bwd / bwd2_chunk by hand; rd_debug_graph_beta_route must report them (and Tc = T for every other LDS case but P19: 30)
ROUTE_TC = {"CAP_T48": (5, 4, 3), "CAP_T64": (5, 4, 3), "CAP_T7": (4, 4, 3), "CAP_T5": (5, 3, 3), "CAP_T125": (42, 42, 42), "P19": (30, 30, 30)}
ROUTE_TC_V1 = {"CAP_T125": 63}                          # rounds 2-5: T halved until it fits; every other V1 case runs one pass
RAGGED = tuple((n, m) for n, tcs in ROUTE_TC.items() for m, tc in zip(MODES, tcs) if tc < CASES[n][2] and CASES[n][2] % tc)

# A case that misses the gap conditions gets another seed here -- never another margin.
SEED_BUMP = {}


def kept_of(E):
    return int(E * 0.5)


def apriori_score_bound(T, ratio=1.0):
    """fp32 bound of one score relative to the score: (T + 34) roundings of 2^-24 times mean|term| / |score|"""
    return (T + 34) * 2.0 ** -24 * ratio


def gap_of(E, T):
    """the margin of a case: 8 x the a-priori bound (all terms positive: ratio 1), or what lets the ladder span LADDER_SPAN (ratio
    1.5 at the most: E <= 3)"""
    return max(8.0 * apriori_score_bound(T), min((LADDER_SPAN ** (1.0 / max(E, 1)) - 1.0) / 2.0, 0.25))


def _rng(*key):
    return np.random.default_rng([zlib.crc32(repr(key).encode()), SEED_BUMP.get(key[0], 0)])


def _graph(rng, kind, N, E):
    """edge_index int64 [2, E] (row 0 source, row 1 target) and the edges that must end up pruned"""
    src, tgt = rng.integers(0, N, size=E), rng.integers(0, N, size=E)
    forced = np.zeros(E, dtype=bool)
    if kind == "no_out":
        owners = np.array([n for n in range(N) if n % 3 != 0])
        src = owners[rng.integers(0, len(owners), size=E)]
        tgt = rng.integers(1, N, size=E)
        tgt[rng.permutation(E)[:E // 10]] = 0               # node 0: in-edges only, every one of them pruned
        forced = tgt == 0
    elif kind == "self":
        tgt = src.copy()
    elif kind == "dup":
        assert E % 2 == 0
        src[E // 2:], tgt[E // 2:] = src[:E // 2], tgt[:E // 2]
    elif kind == "one_src":
        src[:] = N // 2
    elif kind == "one_tgt":
        tgt[:] = N // 2
    return np.stack([src, tgt]).astype(np.int64), forced


def _beta64(H, map_w, p_t):
    """[B, N, T] float64 (construction only; evaluate() has its own statement)"""
    B, N, T, _ = H.shape
    aa = np.concatenate([np.broadcast_to(map_w.astype(np.float64)[None, :, None, :], (B, N, T, 16)),
                         np.broadcast_to(p_t.astype(np.float64)[:, None, :, :], (B, N, T, 16))], axis=-1)
    return (H.astype(np.float64) * aa).mean(-1)


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs of one case (fp32 arrays; treat as read-only)"""
    N, E, T, B, kind, w_ps, pt_ps = CASES[name]
    K, Kk = T * D_OB, kept_of(E)
    rng = _rng(name, N, E, T, B)
    c = dict(name=name, group=GROUP_OF[name], N=N, E=E, T=T, B=B, K=K, Kk=Kk, kind=kind, w_ps=w_ps, pt_ps=pt_ps, gap=gap_of(E, T))
    V = np.maximum(rng.standard_normal((B, N, K)), 0.0).astype(np.float32)
    dout = rng.standard_normal((B, N, K)).astype(np.float32)
    dalpha = rng.standard_normal((B, Kk)).astype(np.float32)
    if kind == "tie":
        ei = np.stack([rng.integers(0, N, size=E), rng.integers(0, N, size=E)]).astype(np.int64)
        c.update(V=V, dout=dout, dalpha=dalpha, ei=ei, H=np.ones((B, N, T, 32), np.float32), map_w=np.full((N, 16), 0.25, np.float32),
                 p_t=np.full((1, T, 16), 0.25, np.float32), w=np.ones((1, E), np.float32))
        return c
    ei, forced = _graph(rng, kind, N, E)
    assert forced.sum() <= E - Kk
    map_w = rng.uniform(0.5, 1.5, size=(N, 16)).astype(np.float32)
    Bp, Bw = (B if pt_ps else 1), (B if w_ps else 1)
    p_t = rng.uniform(0.5, 1.5, size=(Bp, T, 16)).astype(np.float32)
    H = (rng.uniform(0.1, 0.5, size=(B, N, T, 1)) * rng.uniform(0.5, 1.5, size=(B, N, T, 32))).astype(np.float32)
    if not w_ps:                                             # one ladder for every sample: sample b = sample 0 scaled by exact powers of two
        for b in range(1, B):
            kb, jb = (1, -1, 2)[(b - 1) % 3], ((1, -2, 0)[(b - 1) % 3] if pt_ps else 0)
            H[b, ..., :16] = H[0, ..., :16] * np.float32(2.0 ** kb)
            H[b, ..., 16:] = H[0, ..., 16:] * np.float32(2.0 ** (kb - jb))
            if pt_ps:
                p_t[b] = p_t[0] * np.float32(2.0 ** jb)
    beta = _beta64(H, map_w, p_t)
    assert (beta > 0.02).all() and (beta < 1.5 * 4).all()
    s_tgt = beta.mean(-1)[:, ei[1]]                                              # [B, E]
    ratio = 1.0 + 2.0 * c["gap"]
    w = np.empty((Bw, E), dtype=np.float32)
    for b in range(Bw):
        order = rng.permutation(E)
        order = np.concatenate([order[~forced[order]], order[forced[order]]])    # forced-pruned edges take the lowest ranks
        rank = np.empty(E, dtype=np.int64)
        rank[order] = np.arange(E)
        w[b] = (LADDER_TOP * ratio ** (-rank.astype(np.float64)) / s_tgt[b]).astype(np.float32)
    c.update(V=V, dout=dout, dalpha=dalpha, ei=ei, H=H, map_w=map_w, p_t=p_t, w=w, forced=forced)
    return c


def keep_mask(c, seed=DROP_SEED, p=P_DROP):
    """bool [B, E, T, 4]: the mask of rd_graph_beta.h, drawn on the host"""
    return R.edge_coeff_keep(seed, c["B"], c["E"], c["T"], p)


@functools.lru_cache(maxsize=None)
def _mask_of(name):
    return keep_mask(case(name))


def scores(c):
    """float64 [B, E]: the mean score of every edge (the fp32 inputs taken as exact)"""
    beta = _beta64(c["H"], c["map_w"], np.broadcast_to(c["p_t"], (c["B"],) + c["p_t"].shape[1:]))
    w = np.broadcast_to(c["w"].astype(np.float64), (c["B"], c["E"]))
    return (beta[:, c["ei"][1], :] * w[:, :, None]).mean(-1), np.abs(beta[:, c["ei"][1], :] * w[:, :, None]).mean(-1)


def conditions(c):
    """(smallest relative gap between adjacent sorted scores, min |s| / max |s|, the margin required) over the samples"""
    s, absmean = scores(c)
    if c["E"] == 0:
        return np.inf, np.inf, c["gap"]
    ratio = float((absmean / np.abs(s)).max())
    need = max(c["gap"], 8.0 * apriori_score_bound(c["T"], ratio))
    srt = -np.sort(-s, axis=1)
    gaps = ((srt[:, :-1] - srt[:, 1:]) / np.abs(srt[:, :-1])).min() if c["E"] > 1 else np.inf
    return float(gaps), float(np.abs(s).min() / np.abs(s).max()), need


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def _seq_sum(a, axis):
    """running sum along `axis` in a's precision, entries in order"""
    a = np.moveaxis(a, axis, 0)
    s = np.zeros(a.shape[1:], dtype=a.dtype)
    for i in range(a.shape[0]):
        s = s + a[i]
    return s


def evaluate(c, mode="plain", dtype=np.float64, variant=None, keep=None):
    """{out, ei_out, alpha, beta, kept, dV, dH, dmap, dw} of case c in `dtype` (float64: the reference; float32: the yardstick).
    mode: "plain" (no dalpha), "alpha", "drop" (p = P_DROP under `keep`, default the host mask of DROP_SEED, with dalpha).
    variant: one of VARIANTS -- a WRONG kernel, for tests/test_beta_operator_ref_host.py."""
    f = dtype
    B, N, E, T, K = c["B"], c["N"], c["E"], c["T"], c["K"]
    Kk = kept_of(E) if variant != "kk_ceil" else -(-E // 2)
    drop, with_alpha = mode == "drop", mode in ("alpha", "drop")
    if drop and keep is None:
        keep = _mask_of(c["name"])
    inv_keep = f(1.0) / (f(1.0) - f(P_DROP)) if drop else f(1.0)
    V, H, map_w, dout = c["V"].astype(f).reshape(B, N, T, D_OB), c["H"].astype(f), c["map_w"].astype(f), c["dout"].astype(f).reshape(B, N, T, D_OB)
    src, tgt = c["ei"][0], c["ei"][1]
    res = dict(out=np.zeros((B, N, T, D_OB), f), ei_out=np.zeros((B, 2, Kk), np.int64), alpha=np.zeros((B, Kk), f),
               beta=np.zeros((B, N, T), f), kept=np.zeros((B, Kk), np.int32), dV=np.zeros((B, N, T, D_OB), f),
               dH=np.zeros((B, N, T, 32), f), dmap=np.zeros((N, 16), f), dw=np.zeros((B, E), f))
    sc = dict(dH=0.0, dmap=np.zeros((N, 16), f), dw=0.0)                         # max-norms of the same sums over |terms| (error_of)
    for b in range(B):
        p_t = c["p_t"][b if c["pt_ps"] else 0].astype(f)
        w = c["w"][0 if (not c["w_ps"] or variant == "w_stride0") else b].astype(f)
        aa = np.concatenate([np.broadcast_to(map_w[:, None, :], (N, T, 16)), np.broadcast_to(p_t[None, :, :], (N, T, 16))], axis=-1)
        beta = _seq_sum(H[b] * aa, 2) * f(1.0 / 32.0)                             # [N, T]
        res["beta"][b] = beta
        score = _seq_sum(beta[tgt] * w[:, None], 1) / f(T) if E else np.zeros(0, f)
        order = np.argsort(-score, kind="stable")                                 # descending, ties: lower edge id first
        if variant == "pad_key" and b == 0:                                       # a pad key in front of the last kept real key
            order = np.concatenate([order[:Kk - 1], order[-1:], order[Kk - 1:-1]])
        kept = order[:Kk]
        ks, kt, kw = src[kept], tgt[kept], w[kept]
        res["kept"][b], res["ei_out"][b, 0], res["ei_out"][b, 1], res["alpha"][b] = kept, ks, kt, score[kept]
        if Kk == 0:
            continue
        g = beta[kt] * kw[:, None]                                                # [Kk, T]
        grp = kt if variant == "per_target" else ks                               # the softmax's groups
        active = np.ones(Kk, dtype=bool)
        if variant == "drop_pos64":
            active[64] = False
        ga = np.where(active[:, None], g, -np.inf)
        m = np.full((N, T), -np.inf, f)
        np.maximum.at(m, grp, ga)
        scale = np.ones((Kk, T, D_OB), f)
        if drop:
            scale = keep[b, np.arange(Kk) if variant == "mask_by_pos" else kept].astype(f) * inv_keep
        with np.errstate(invalid="ignore"):
            ex = np.where(active[:, None], np.exp(ga - m[grp]), f(0.0)).astype(f)
        if variant == "mask_before_norm":
            z = np.zeros((N, T, D_OB), f)
            np.add.at(z, grp, ex[:, :, None] * scale)
            C = ex[:, :, None] * scale / (z[grp] + f(1e-16))
            P = ex / (z[grp].max(-1) + f(1e-16))
        else:
            z = np.zeros((N, T), f)
            np.add.at(z, grp, ex)
            P = ex * (f(1.0) / (z[grp] + f(1e-16)))
            C = P[:, :, None] * scale
        np.add.at(res["out"][b], ks, C * V[b, kt])
        # backward
        do = dout[b, ks]                                                          # [Kk, T, 4]
        np.add.at(res["dV"][b], kt, C * do)
        dP = _seq_sum(scale * do * V[b, kt], 2)
        S = np.zeros((N, T), f)
        np.add.at(S, grp, P * dP)
        dg = P * (dP - S[grp])
        dbeta = np.zeros((N, T), f)
        np.add.at(dbeta, kt, kw[:, None] * dg)
        dgw = dg * beta[kt]
        db_sum = dbeta
        if variant == "skip_chunk_last":                                          # step CHUNK_TC - 1 never reaches the sums over time
            dgw = dgw.copy()
            dgw[:, CHUNK_TC - 1] = 0
        dwk = _seq_sum(dgw, 1)
        if with_alpha:
            da = c["dalpha"][b, :Kk].astype(f) if c["dalpha"].shape[1] >= Kk else np.zeros(Kk, f)
            cb = np.zeros(N, f)
            np.add.at(cb, kt, da * kw)
            dbeta = dbeta + (cb / f(T))[:, None]
            db_sum = dbeta
            if variant != "no_dalpha_dw":
                dwk = dwk + da * (_seq_sum(beta, 1)[kt] / f(T))
        db = dbeta * f(1.0 / 32.0)
        res["dH"][b] = db[:, :, None] * aa
        dbm = db
        if variant == "skip_chunk_last":
            dbm = db.copy()
            dbm[:, CHUNK_TC - 1] = 0
        res["dmap"] += _seq_sum(dbm[:, :, None] * H[b, :, :, :16], 1)
        np.add.at(res["dw"][b], kept, dwk)                                        # (kept ids are distinct: a plain store)
        # the same sums with every term's absolute value: what the softmax backward's dP - S cancels against
        S_abs = np.zeros((N, T), f)
        np.add.at(S_abs, grp, P * np.abs(dP))
        dg_abs = P * (np.abs(dP) + S_abs[grp])
        dbeta_abs = np.zeros((N, T), f)
        np.add.at(dbeta_abs, kt, kw[:, None] * dg_abs)
        dw_abs = (dg_abs * np.abs(beta[kt])).sum(1)
        if with_alpha:
            cb_abs = np.zeros(N, f)
            np.add.at(cb_abs, kt, np.abs(da * kw))
            dbeta_abs = dbeta_abs + (cb_abs / f(T))[:, None]
            dw_abs = dw_abs + np.abs(da) * np.abs(beta).sum(1)[kt] / f(T)
        sc["dH"] = max(sc["dH"], float((dbeta_abs[:, :, None] * np.abs(aa)).max()) / 32.0)
        sc["dmap"] += (dbeta_abs[:, :, None] * np.abs(H[b, :, :, :16])).sum(1) / f(32.0)
        sc["dw"] = max(sc["dw"], float(dw_abs.max()))
    if variant == "kk_ceil":                                                      # the lists in the caller's [.., int(E/2)] buffers
        k0 = kept_of(E)
        res["ei_out"], res["alpha"], res["kept"] = res["ei_out"][:, :, :k0], res["alpha"][:, :k0], res["kept"][:, :k0]
    res["out"], res["dV"] = res["out"].reshape(B, N, K), res["dV"].reshape(B, N, K)
    res["dH"] = res["dH"].reshape(B, N, T * 32)
    res["scale"] = dict(dH=sc["dH"], dmap=float(sc["dmap"].max()), dw=sc["dw"])
    return res


# variant -> (case, mode): each must miss some working bound by 10 x (tests/test_beta_operator_ref_host.py)
VARIANTS = {
    "drop_pos64": ("KK65", "plain"),           # position 64 of a 65-entry kept list dropped from its source's list
    "per_target": ("N17", "plain"),            # the softmax normalised per target
    "kk_ceil": ("KK64", "plain"),              # Kk = ceil(E / 2) at E = 129
    "skip_chunk_last": (CHUNK_CASE, "plain"),  # the last step of the first backward chunk left out of d map_w and dw
    "no_dalpha_dw": ("N33", "alpha"),          # the dalpha term left out of dw
    "mask_by_pos": ("KK63", "drop"),           # the mask indexed by kept position
    "mask_before_norm": ("N16", "drop"),       # the mask applied before the softmax normaliser
    "pad_key": ("H_E4097", "plain"),           # one pad key sorted in front of a real key at E = 4097
    "w_stride0": ("S_WP_PS", "plain"),         # w read with stride 0 where it is per-sample
}

_REF = {}


def reference(name, mode, dtype=np.float64):
    """evaluate() of a case, computed once per (case, mode, precision) and shared: callers must not modify it"""
    key = (name, mode, np.dtype(dtype).name)
    if key not in _REF:
        _REF[key] = evaluate(case(name), mode, dtype)
    return _REF[key]


# ---- errors and bounds --------------------------------------------------------------------------------------------------------------------
CANCELLED = 1e-3


def error_of(tensor, got, ref, scale=None):
    """error of `got` in the tensor's metric: max |difference|, over the reference's max-norm for everything but `out`.
    scale (dH, dmap, dw): the max-norm of the same sums over the terms' absolute values (evaluate()'s "scale").  Where every kept edge
    of a source shares its target (N = 1, self-loops only) the softmax backward's dP - S is zero in exact arithmetic -- the float64
    gradient is the 1e-16 of the normaliser, and an error relative to THAT norm measures nothing.  So a gradient whose float64
    max-norm is under CANCELLED = 1e-3 of `scale` is compared relative to `scale`: the terms any implementation has to cancel."""
    a, r = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == r.shape, (tensor, a.shape, r.shape)
    if a.size == 0:
        return 0.0
    e = float(np.abs(a - r).max())
    if tensor != "out":
        norm = float(np.abs(r).max())
        if scale is not None and norm < CANCELLED * scale:
            norm = scale
        e = e / norm if norm > 0 else (0.0 if e == 0 else np.inf)
    return e if np.isfinite(a).all() else np.inf


def ceiling_of(tensor, mode):
    return CEILING[tensor] * (1.0 / (1.0 - P_DROP) if mode == "drop" and tensor == "out" else 1.0)


@functools.lru_cache(maxsize=None)
def yardstick(group, mode):
    """tensor -> (largest error of the float32 evaluation against the float64 one over the group's cases, the case)"""
    worst = {t: (0.0, None) for t in COMPARED}
    for name in GROUPS[group]:
        r64, r32 = reference(name, mode), reference(name, mode, np.float32)
        assert np.array_equal(r64["kept"], r32["kept"]), (name, "the gap must keep the float32 order")
        for t in COMPARED:
            e = error_of(t, r32[t], r64[t], r64["scale"].get(t))
            if e > worst[t][0]:
                worst[t] = (e, name)
    return worst


def bound_of(tensor, group, mode, norm=1.0):
    """working bound of a compared tensor: min(ceiling, max(4 x the CPU yardstick of the group, 8 x 2^-24 of the norm)); norm: max
    |reference| for `out` (compared in absolute terms), 1 for the relative metrics.  Takes the ceilings and the CPU yardstick only."""
    floor = FLOOR * (norm if tensor == "out" else 1.0)
    return min(ceiling_of(tensor, mode), max(YARD_FACTOR * yardstick(group, mode)[tensor][0], floor))


def norm_of(tensor, ref):
    return float(np.abs(ref[tensor]).max()) if tensor == "out" and ref[tensor].size else 1.0


def compare(name, mode, got, ref=None):
    """[(tensor, error, bound)] of every compared tensor of a run + whether the lists are bit-equal"""
    c = case(name)
    ref = reference(name, mode) if ref is None else ref
    rows = [(t, error_of(t, got[t], ref[t], ref["scale"].get(t)), bound_of(t, c["group"], mode, norm_of(t, ref))) for t in COMPARED]
    lists_ok = all(np.array_equal(np.asarray(got[t]).astype(np.int64), ref[t].astype(np.int64)) for t in LISTS)
    return rows, lists_ok


def variant_margin(variant):
    """largest error / working bound over the compared tensors of the wrong kernel `variant` (inf where a list differs)"""
    name, mode = VARIANTS[variant]
    rows, lists_ok = compare(name, mode, evaluate(case(name), mode, variant=variant))
    if not lists_ok:
        return np.inf
    return max(e / b if b > 0 else (np.inf if e > 0 else 0.0) for _, e, b in rows)
