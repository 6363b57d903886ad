"""CPU: the host restatement of the dropout generator (tests/rng_ref.py) against the published Threefry vectors, its element
numbering, and the condition that makes tests/test_dropout_reference_gpu.py worth running: a wrong mask moves the float64
references (tests/dropout_ref.py) by at least 20 x the bounds the kernels are held to."""
import numpy as np
import pytest

from tests import dropout_ref as DR
from tests import rng_ref as R


@pytest.mark.parametrize("counter,key,out", [
    ((0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x9d1c5ec6, 0x8bd50731)),
    ((0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0xfd36d048, 0x2d17272c)),
    ((0x243f6a88, 0x85a308d3), (0x13198a2e, 0x03707344), (0xba3e4725, 0xf27d669e))])
def test_threefry2x32_13_known_answers(counter, key, out):
    """Random123's known-answer vectors of threefry2x32 with 13 rounds (kat_vectors: zeros, ones, digits of pi)."""
    x0, x1 = R.threefry2x32_13(counter[0], counter[1], key[0], key[1])
    assert (int(x0), int(x1)) == out


def test_uniform4_is_the_header_s_statement():
    """counter = (quad low word, quad high word | site << 16), key = the seed's words, components = the four 16-bit halves in the
    header's order, times 2^-16; vectorised evaluation equals the scalar one."""
    seed, site, quad = (5 << 32) | 77, 33, (3 << 32) | 123456
    x0, x1 = R.threefry2x32_13(123456, 3 | (33 << 16), 77, 5)
    want = np.array([int(x0) & 0xFFFF, int(x0) >> 16, int(x1) & 0xFFFF, int(x1) >> 16], dtype=np.float32) / np.float32(65536.0)
    assert np.array_equal(R.uniform4(seed, site, quad), want)
    quads = np.array([0, 1, quad, 2 ** 40 + 9], dtype=np.uint64)
    u = R.uniform4(seed, site, quads)
    assert u.shape == (4, 4) and u.dtype == np.float32 and np.array_equal(u[2], want)
    idx = np.arange(64)
    k = R.keep(seed, site, idx, 0.5)
    assert np.array_equal(k, (R.uniform4(seed, site, idx >> 2)[np.arange(64), idx & 3] >= np.float32(0.5)))
    assert not np.array_equal(R.uniform4(seed, site, quads), R.uniform4(seed, site + 1, quads))          # the site enters
    assert not np.array_equal(R.uniform4(seed, site, quads), R.uniform4(seed + (1 << 32), site, quads))  # and the seed's high word


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_keep_fraction(p):
    """2^20 decisions keep 1 - p of the elements within 4 sigma (sigma = sqrt(p (1-p) / n))."""
    n = 1 << 20
    frac = R.keep(77, R.SITE_FFN_HID + 1, np.arange(n), p).mean()
    assert abs(frac - (1.0 - p)) < 4.0 * np.sqrt(p * (1.0 - p) / n), frac


def test_index_helpers_are_injective():
    """No two elements of a site share a (quad, component); T is no multiple of 4."""
    T, B, F, d, H = 7, 3, 5, 4, 2
    idx = R.obs_embed_index(T, B, F, d)
    assert idx.shape == (T, B, F * d) and np.array_equal(idx.reshape(-1), np.arange(T * B * F * d))    # h's own [T, B, F*d] order
    rows = R.padded_rows(T, B)
    assert np.array_equal(np.sort(rows.reshape(-1)), np.arange(T * B))
    for N in (36, 40):
        e = R.row_local_index(rows, N)
        assert e.shape == (T, B, N) and len(np.unique(e)) == e.size and e.max() == T * B * N - 1
    lengths = np.array([3, 7, 1, 7, 5])
    pl = DR.plan_ref(lengths, T)
    prow = R.plan_rows(pl["off"], pl["rank"], T)
    live = np.arange(T)[:, None] < lengths[None, :]
    assert np.array_equal(np.sort(prow[live]), np.arange(lengths.sum()))            # the live rows tile 0 .. M_live exactly once
    assert prow[0, 1] == 0 and prow[0, 3] == 7 and prow[0, 4] == 14                  # longest first, ties by sample index
    for rank in (None, pl["rank"]):
        Bx = B if rank is None else len(lengths)
        bh = R.attn_bh(Bx, H, rank)
        assert np.array_equal(np.sort(bh.reshape(-1)), np.arange(Bx * H))
        quad, comp = R.attn_quad(bh[:, :, None, None], T, np.arange(T)[None, None, :, None], np.arange(T)[None, None, None, :])
        flat = (quad * 4 + comp).reshape(-1)
        assert len(np.unique(flat)) == Bx * H * T * T and quad.max() == Bx * H * T * ((T + 3) // 4) - 1
    assert R.attn_bh(5, H, pl["rank"])[1, 0] == 0 and R.attn_bh(5, H)[1, 0] == H     # a plan numbers the masks by rank


def _margins(ref_fn, bound_fn):
    ref = ref_fn(None)
    return {(v, mode): DR.variant_margin(ref, ref_fn(v), bound_fn(mode)) for v in DR.VARIANTS for mode in DR.MODES}


@pytest.mark.parametrize("layer", [0, 1])
def test_wrong_masks_move_the_attention_reference(layer):
    """3b on (33, 4, 34, 2): the mask shifted by one element, 1/(1-p) left out, sample 0's mask for every sample and the other
    layer's site each move out / dqkv by at least 20 x the attention bounds of either mode (lse does not depend on the mask)."""
    m = _margins(lambda v: DR.attn_reference(33, 4, 34, 2, layer, v), DR.attn_bound)
    assert min(m.values()) >= 20.0, m


@pytest.mark.parametrize("layer", [0, 1])
def test_wrong_masks_move_the_encoder_layer_reference(layer):
    """3c on (7, 3, 5, 2): the same four variants against the encoder-layer bounds of either mode."""
    m = _margins(lambda v: DR.enc_reference(7, 3, 5, 2, layer, v), DR.enc_bound)
    assert min(m.values()) >= 20.0, m


def test_each_site_of_the_encoder_layer_is_seen():
    """Flipping ONE site's statement at a time (its `+ layer` dropped, i.e. layer 0's site in layer 1) moves the encoder-layer
    reference by at least 20 x the bounds: no site hides behind the others."""
    T, B, F, H = 7, 3, 5, 2
    c = DR.enc_case(T, B, F, H)
    ref = DR.enc_reference(T, B, F, H, 1)
    import torch
    from oracle import restatement as O2
    right = DR.Masks(DR.SEED, DR.P_DROP, T, B).encoder(1, H, c["D"], c["nhid"])
    wrong = DR.Masks(DR.SEED, DR.P_DROP, T, B).encoder(0, H, c["D"], c["nhid"])
    for i in range(4):
        scales = list(right)
        scales[i] = wrong[i]
        xr = c["x"].double().requires_grad_(True)
        pr = {("L." + n): t.double().requires_grad_(True) for n, t in c["p"].items()}
        y = O2.encoder_layer(xr, c["mask"], pr, "L.", H, drop=DR.DropHook(scales))
        g = torch.autograd.grad(y, [xr] + [pr["L." + n] for n in DR.ENC_NAMES], c["dy"].double())
        got = dict(y=y.detach().numpy())
        got.update((n, t.numpy()) for n, t in zip(("x",) + DR.ENC_NAMES, g))
        for mode in DR.MODES:
            assert DR.variant_margin(ref, got, DR.enc_bound(mode)) >= 20.0, (i, mode)
