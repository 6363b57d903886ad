"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the dropout generator (raindrop_amd/csrc/rd_rng.h) and of the element numbering
of every dropout site family, so that a float64 reference can apply the very masks the kernels draw.

A keep decision is a pure function of (seed + seed cell, site, element): Threefry-2x32 with 13 rounds, one call per element quad,
16 random bits per element, keep iff float32(u) >= float32(p).  tests/test_dropout_reference_gpu.py ties this file to the device
generator bit for bit through rd_scale_dropout; tests/test_rng_ref_host.py holds the published known-answer vectors."""
import numpy as np

# rd_rng.h `enum DropSite`; the encoder sites take `+ layer`
SITE_OBS_EMBED, SITE_EDGE_COEFF, SITE_ATTN_PROB, SITE_ATTN_OUT, SITE_FFN_HID, SITE_FFN_OUT = 1, 2, 16, 32, 48, 64

_M32 = np.uint64(0xFFFFFFFF)
_ROT = (13, 15, 26, 6, 17, 29, 16, 24)


def _u64(x):
    return np.asarray(x).astype(np.uint64)


def threefry2x32_13(c0, c1, k0, k1):
    """Random123 threefry2x32_R(13, counter, key) -- rd_rng.h:34-47.  32-bit words (arrays broadcast); returns (x0, x1) as uint64
    arrays holding 32-bit values."""
    c0, c1, k0, k1 = (_u64(v) & _M32 for v in (c0, c1, k0, k1))
    ks = (k0, k1, np.uint64(0x1BD11BDA) ^ k0 ^ k1)
    x0 = (c0 + ks[0]) & _M32
    x1 = (c1 + ks[1]) & _M32
    for r in range(13):
        x0 = (x0 + x1) & _M32
        rot = np.uint64(_ROT[r & 7])
        x1 = ((x1 << rot) | (x1 >> (np.uint64(32) - rot))) & _M32
        x1 = x1 ^ x0
        if ((r + 1) & 3) == 0:
            s = (r + 1) >> 2
            x0 = (x0 + ks[s % 3]) & _M32
            x1 = (x1 + ks[(s + 1) % 3] + np.uint64(s)) & _M32
    return x0, x1


def uniform4(seed, site, quad):
    """The four uniforms k * 2^-16 of element quad `quad` of `site` under `seed` -- rd_rng.h:50-62 (the Threefry branch): counter
    (quad & 0xffffffff, (quad >> 32) | (site << 16)), key (seed low word, seed high word); components in the header's order
    x0 & 0xffff, x0 >> 16, x1 & 0xffff, x1 >> 16.  float32 [..., 4]."""
    quad = _u64(quad)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c1 = (quad >> np.uint64(32)) | np.uint64((int(site) << 16) & 0xFFFFFFFF)
    x0, x1 = threefry2x32_13(quad & _M32, c1, np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    h = np.uint64(0xFFFF)
    u = np.stack([x0 & h, x0 >> np.uint64(16), x1 & h, x1 >> np.uint64(16)], axis=-1)
    return u.astype(np.float32) * np.float32(1.0 / 65536.0)


def keep_quad(seed, site, quad, comp, p):
    """bool: component `comp` (0..3) of quad `quad` is kept -- the `v >= p` of rd_rng.h:70 in float32."""
    u = uniform4(seed, site, quad)
    comp = np.broadcast_to(np.asarray(comp, dtype=np.int64), u.shape[:-1])
    return np.take_along_axis(u, comp[..., None], axis=-1)[..., 0] >= np.float32(p)


def keep(seed, site, idx, p):
    """bool: element `idx` of `site` is kept -- dropout_scale, rd_rng.h:65-71: quad idx >> 2, component idx & 3."""
    idx = _u64(idx)
    return keep_quad(seed, site, idx >> np.uint64(2), (idx & np.uint64(3)).astype(np.int64), p)


def site_of(family, layer=0):
    """Site number of an encoder family in layer `layer` (rd_temporal.hip rd_encoder_layer_fwd / _bwd: SITE_x + L)."""
    return int(family) + int(layer)


# ---------------------------------------------------------------------------------------------------------------------------------
# element numbering, one helper per site family
# ---------------------------------------------------------------------------------------------------------------------------------


def obs_embed_index(T, B, F, d):
    """int64 [T, B, F*d]: element ((t*B + b)*F + f)*d + c of h in its own [T, B, F*d] order -- rd_msgpass.hip:45 (k_obs_embed) and,
    as quad (t*B + b)*F + f with the four channels c as components (d = 4), rd_msgpass_fused.hip:581.  `b` is the caller's sample
    index on the padded layout AND on a token plan (rd_msgpass_fused.hip:86-89: `b` indexes the caller's tensors)."""
    t = np.arange(T, dtype=np.int64)[:, None, None, None]
    b = np.arange(B, dtype=np.int64)[None, :, None, None]
    f = np.arange(F, dtype=np.int64)[None, None, :, None]
    c = np.arange(d, dtype=np.int64)[None, None, None, :]
    return (((t * B + b) * F + f) * d + c).reshape(T, B, F * d)


def padded_rows(T, B):
    """int64 [T, B]: row t*B + b of a [T, B, *] tensor (rd_attention.hip:58: "row of step t = t*B + b")."""
    return np.arange(T, dtype=np.int64)[:, None] * B + np.arange(B, dtype=np.int64)[None, :]


def plan_rows(off, rank, T):
    """int64 [T, B]: row off[rank[b]] + t of step t of sample b on a token plan (rd_attention.hip:59-60, rd_plan.h: the rows of
    the sample of rank r are the block off[r] .. off[r] + len[r]).  Entries with t >= len[b] name rows of other samples: the
    caller masks them out (those steps do not exist on the plan)."""
    off, rank = np.asarray(off, dtype=np.int64), np.asarray(rank, dtype=np.int64)
    return off[rank][None, :] + np.arange(T, dtype=np.int64)[:, None]


def row_local_index(rows, N):
    """int64 [..., N]: element row*N + c of the row-local sites (attention output and FFN output: N = D; FFN hidden: N = nhid) --
    rd_layernorm.hip:33 / 145 (add + LayerNorm), rd_gemm.hip:97 / 412, rd_rowgemm.hip:240 / 415 / 449, rd_encfuse.hip:336 / 507 /
    689."""
    rows = np.asarray(rows, dtype=np.int64)
    return rows[..., None] * int(N) + np.arange(int(N), dtype=np.int64)


def attn_bh(B, H, rank=None):
    """int64 [B, H]: the (sample, head) number of the attention masks: b*H + h with b the SAMPLE index on the padded layout
    (rd_attention.hip:182: bh = blockIdx.y, b = bh / H) and the sample's RANK on a token plan (rd_attention.hip:59 "workgroup index b
    is a RANK", rd_attnfuse.hip:22 / 360: attn_quad(rank * H + h, ..))."""
    b = np.arange(B, dtype=np.int64) if rank is None else np.asarray(rank, dtype=np.int64)
    return b[:, None] * H + np.arange(H, dtype=np.int64)[None, :]


def attn_quad(bh, T, q, key):
    """(quad, component) of probability (bh, q, key): quad (bh*T + key)*ceil(T/4) + (q >> 2), component q & 3 --
    rd_attention.hip:78-80 (attn_quad) and :81-87 (attn_keep1)."""
    bh, q, key = (np.asarray(v, dtype=np.int64) for v in (bh, q, key))
    return (bh * T + key) * ((T + 3) >> 2) + (q >> 2), q & 3


def attn_keep(seed, site, bh, T, p):
    """bool [B, H, T(query), T(key)] keep decisions of the attention probabilities for the [B, H] numbers `bh` (attn_bh)."""
    bh = np.asarray(bh, dtype=np.int64)[:, :, None, None]
    q = np.arange(T, dtype=np.int64)[None, None, :, None]
    key = np.arange(T, dtype=np.int64)[None, None, None, :]
    quad, comp = attn_quad(bh, T, q, key)
    return keep_quad(seed, site, quad, comp, p)


def edge_coeff_quad(B, E, T):
    """int64 [B, E, T]: quad (b*E + e)*T + t of the use_beta branch's coefficient dropout, e the edge's id in the INPUT list (not
    its position among the kept ones) -- rd_graph_beta.h beta_drop_base; the four uniforms of the quad are the d_ob = 4 channels."""
    b = np.arange(B, dtype=np.int64)[:, None, None]
    e = np.arange(E, dtype=np.int64)[None, :, None]
    t = np.arange(T, dtype=np.int64)[None, None, :]
    return (b * E + e) * T + t


def edge_coeff_keep(seed, B, E, T, p):
    """bool [B, E, T, 4]: channel c of (sample, input edge, step) is kept -- rd_graph_beta.h beta_keep_code at SITE_EDGE_COEFF: u >= p
    in float32, what rd_graph_beta_keep writes as bytes."""
    return uniform4(seed, SITE_EDGE_COEFF, edge_coeff_quad(B, E, T)) >= np.float32(p)
