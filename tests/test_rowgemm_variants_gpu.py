"""GPU: every instantiation of the encoder's row-block product (raindrop_amd/csrc/rd_rowgemm.hip k_rowgemm) and every variant of
the fused row-local chains (rd_encfuse.hip) that a process-global knob or an environment switch can select.

k_rowgemm is built 21 times (workgroup height 32 / 64 rows x 8 / 16 waves, for the plain product at two reduction lengths, the
LayerNorm epilogue and the LayerNorm-backward prologue, + the K = 3D product); two masks (rd_set_rowgemm_rows32 /
rd_set_rowgemm_waves16) choose among them, and TrainStep's autotune leaves the pair that won on the box of the run set for the rest
of the process.  The rest of the suite runs the default pair only.  Here the layer is forced onto the row-block launches
(RD_ENC_FUSE=0, RD_ATTN_FUSE=0, both read per call) and run under every pair of SETTINGS:

  1. against the default pair on the same inputs, dropout off and on: the masks change which rows share a workgroup, never a
     row's arithmetic -- bit-identical output, input gradient and weight / bias gradients; the four LayerNorm affine gradients
     (per-workgroup partials, grouped by the block height) within 2e-5 of their max-norm;
  2. the default pair against the float64 restatement at the same shapes.

tests/test_rowgemm_variants_host.py checks (without a GPU) that SETTINGS selects all 21 instantiations and holds every pair the
autotune can choose.  The second half of the file compares the fused chains' own variants (RD_ENC_SPECIALIZE, RD_ENC_FUSE_TALL,
RD_ENC_LEAN) with their defaults."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from oracle import restatement as O2
from raindrop_amd import synth
from raindrop_amd.step import TrainStep

pytestmark = pytest.mark.gpu
DEV = "cuda"

REFERENCE = (15, 12)                                  # (rows32 mask, waves16 mask): the library's defaults
CORNERS = [(0, 0), (15, 0), (0, 15), (15, 15)]        # between them every rows x waves form of every kernel class
TUNED = [(h, w) for h in TrainStep.TUNE_HEIGHTS for w in TrainStep.TUNE_WAVES]      # what TrainStep._capture can leave behind
SETTINGS = list(dict.fromkeys(CORNERS + TUNED))

# (F, D, nhid): D = 4 F + 16.  rowgemm_ok needs ceil(K / 32) of 5, 9 and 15 for K = D, nhid and 3 D, every width a multiple of 4, and
# the LayerNorm epilogue D <= 256 (rd_temporal.hip enc_route: `rg`, `tw`, `lnf1/lnf2`, `lnb`):
#   152 / 272 / 456 -> 5 / 9 / 15 (P19);  160 / 288 / 480 -> 5 / 9 / 15 (P12: no padding column in any plane);
#   156 / 260 / 468 -> 5 / 9 / 15: not compiled into any chain; N = 260 leaves 4 valid columns in a plain product's second round,
#   N = 468 (in_proj) 212 of 256.
WIDTHS = [(34, 152, 272), (36, 160, 288), (35, 156, 260)]
# (T, B): M = T B rows against the 32- and 64-row blocks -- 21 (< 32), 32, 33, 63, 65, 360 (= 40 mod 64), 999, and T = 70 > 64 (the
# multi-tile attention next to 210 ragged rows)
SMALL = [(7, 3), (8, 4), (11, 3), (21, 3), (13, 5), (60, 6), (37, 27), (70, 3)]
LARGE = (60, 256)                                     # 15360 rows: 240 / 480 workgroups, more than one round on 256 CUs; corners only
ENC_NAMES = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
             "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
             "norm2.bias")
LN_AFFINE = ("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")
GATE_FREE = ("linear2.weight", "linear2.bias", "norm2.weight", "norm2.bias")      # continuous in the ReLU gates (h ~ 0 at a flip)


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _rel2(a, b):
    return float(np.linalg.norm((a - b).ravel().astype(np.float64)) / (np.linalg.norm(b.ravel().astype(np.float64)) + 1e-30))


def _set_masks(rows32, waves16):
    from raindrop_amd import _lib
    _lib.call("rd_set_rowgemm_rows32", rows32)
    _lib.call("rd_set_rowgemm_waves16", waves16)


@pytest.fixture(autouse=True)
def _explicit_masks_and_row_block_path(monkeypatch):
    """Both masks are set explicitly before each test and handed back to the environment / default (-1) afterwards: these tests
    neither depend on nor leak the process-global choice (a TrainStep built earlier in the process leaves its autotune's winner
    set).  Arithmetic mode 1 (split-bf16) is restored as well."""
    from raindrop_amd import _lib, ops
    assert ENC_NAMES == tuple(ops.ENC_PARAM_NAMES)
    _set_masks(*REFERENCE)
    _lib.call("rd_set_precision", 1)
    try:
        yield
    finally:
        _set_masks(-1, -1)
        _lib.call("rd_set_precision", 1)


@pytest.fixture(scope="module", autouse=True)
def _hand_back_device_memory():
    """The steps and models built below sit in reference cycles, and the 15360-row cases leave large blocks in torch's caching
    allocator.  Collected whenever the interpreter next happens to, they would free device blocks in the middle of a LATER module's
    test -- and tests/test_step_launches_gpu.py names buffers by the order in which their addresses first appear, so which freed block
    an allocation reuses is part of what it compares.  Collect and release here: this module leaves the allocator without garbage of
    its own."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


class _Stamps:
    """A zeroed device buffer registered with one of the debug setters of include/raindrop_hip_debug.h: the launchers pass it to the
    kernels as an argument, which write clock values into it -- non-zero afterwards = the kernels of that file really ran."""

    def __init__(self, setter, words):
        from raindrop_amd import _lib
        self.fn = getattr(_lib.load(), setter)
        self.fn.argtypes, self.fn.restype = [ctypes.c_void_p], None
        self.buf = torch.zeros(words, dtype=torch.int64, device=DEV)

    def __enter__(self):
        self.fn(ctypes.c_void_p(self.buf.data_ptr()))
        return self

    def __exit__(self, *exc):
        self.fn(None)
        torch.cuda.synchronize()

    def take(self):
        """host copy of the buffer; the buffer is zeroed for the next run"""
        torch.cuda.synchronize()
        v = self.buf.cpu().numpy().copy()
        self.buf.zero_()
        return v


def _rowgemm_stamps():
    return _Stamps("rd_debug_set_rowgemm_stamps", 8 * 16)          # wave 0 of the first 8 workgroups, 16 phases (RGSTAMP)


def _encfuse_stamps():
    return _Stamps("rd_debug_set_encfuse_stamps", 8192)            # forward chain [0, 4096), backward chain [4096, 8192)


def _enc_params(D, nhid, seed):
    shapes = {"self_attn.in_proj_weight": (3 * D, D), "self_attn.in_proj_bias": (3 * D,), "self_attn.out_proj.weight": (D, D),
              "self_attn.out_proj.bias": (D,), "linear1.weight": (nhid, D), "linear1.bias": (nhid,), "linear2.weight": (D, nhid),
              "linear2.bias": (D,), "norm1.weight": (D,), "norm1.bias": (D,), "norm2.weight": (D,), "norm2.bias": (D,)}
    return {n: synth.param_values("L." + n, shapes[n], seed=seed) for n in ENC_NAMES}


def _layer_inputs(T, B, D, nhid, seed):
    """x, key-padding mask of ragged lengths (lengths[0] = T), dy, parameters -- on the host"""
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((T, B, D)).astype(np.float32))
    lengths = torch.from_numpy(rng.integers(1, T + 1, size=B)).long()
    lengths[0] = T
    mask = torch.from_numpy(O2.padding_mask(lengths.numpy(), T))
    dy = torch.from_numpy(rng.standard_normal((T, B, D)).astype(np.float32))
    return x, mask, dy, _enc_params(D, nhid, seed=T)


def _run_layer(x, mask, dy, p, shp, p_drop, seed=77):
    """ops.encoder_layer forward + backward on device tensors -> (y, [dx, 12 parameter gradients]) as numpy"""
    from raindrop_amd import ops
    xd = x.clone().requires_grad_(True)
    pd = [p[n].clone().requires_grad_(True) for n in ENC_NAMES]
    y = ops.encoder_layer(xd, mask, shp, 1, p_drop, seed, pd)
    g = torch.autograd.grad(y, [xd] + pd, dy)
    torch.cuda.synchronize()
    return y.detach().cpu().numpy(), [t.cpu().numpy() for t in g]


def _to_dev(x, mask, dy, p):
    return x.to(DEV), mask.to(DEV), dy.to(DEV), {n: t.to(DEV) for n, t in p.items()}


def _force_row_blocks(monkeypatch):
    monkeypatch.setenv("RD_ENC_FUSE", "0")
    monkeypatch.setenv("RD_ATTN_FUSE", "0")


SHAPE_CASES = [(T, B, SETTINGS) for T, B in SMALL] + [LARGE + (CORNERS,)]


@pytest.mark.parametrize("mode", [1, 2], ids=["bf16x3", "bf16"])
@pytest.mark.parametrize("F,D,nhid", WIDTHS, ids=["%dx%d" % (d, h) for _, d, h in WIDTHS])
@pytest.mark.parametrize("T,B,settings", SHAPE_CASES, ids=["T%dB%d" % (t, b) for t, b, _ in SHAPE_CASES])
def test_every_mask_setting_matches_the_default_masks(T, B, settings, F, D, nhid, mode, monkeypatch):
    """Assertion 1.  One encoder layer on the row-block launches (in_proj N = 3D: two 256-column rounds, the second ragged;
    out_proj + LayerNorm1; linear1; linear2 + LayerNorm2; both LayerNorm-backward prologues; every input-gradient product; the
    K = 3D product), in the split-bf16 and the single-product bf16 mode, dropout off and on (p = 0.2, fixed seed), under every mask
    pair of `settings` against REFERENCE on the same inputs.
    Bit-identical: y, dx and the gradients of in_proj, out_proj, linear1 and linear2 (weights and biases) -- each LayerNorm row is
    one wave's 64-lane sum whatever the block, the dropout quad is a function of (seed, site, row, column), the exported operand
    tiles hold the same values in the same 32-row chunks.  norm1 / norm2 weight and bias: per-workgroup partials grouped by
    RG_ROWS / WV rows per wave and by block -- a pure change of fp32 summation order, 2e-5 of the tensor's max-norm.
    The row-block stamps must be written in every run (the launches really were k_rowgemm)."""
    from raindrop_amd import _lib
    assert D == 4 * F + 16
    _force_row_blocks(monkeypatch)
    _lib.call("rd_set_precision", mode)
    x, mask, dy, p = _to_dev(*_layer_inputs(T, B, D, nhid, seed=T * 31 + B))
    shp = _lib.shape(B, T, F, 4, nhead=2, nhid=nhid)
    with _rowgemm_stamps() as st:
        for p_drop in (0.0, 0.2):
            _set_masks(*REFERENCE)
            y0, g0 = _run_layer(x, mask, dy, p, shp, p_drop)
            assert st.take().any(), "reference run: no k_rowgemm launch"
            assert np.isfinite(y0).all() and all(np.isfinite(t).all() for t in g0)
            for rows32, waves16 in settings:
                if (rows32, waves16) == REFERENCE:
                    continue
                _set_masks(rows32, waves16)
                y1, g1 = _run_layer(x, mask, dy, p, shp, p_drop)
                tag = "masks (%d, %d), p_drop %.1f" % (rows32, waves16, p_drop)
                assert st.take().any(), tag + ": no k_rowgemm launch"
                assert np.array_equal(y1, y0), (tag, "y", _rel(y1, y0))
                for name, a, r in zip(("x",) + ENC_NAMES, g1, g0):
                    if name in LN_AFFINE:
                        assert _rel(a, r) <= 2e-5, (tag, name, _rel(a, r))
                    else:
                        assert np.array_equal(a, r), (tag, name, _rel(a, r))


F64_CASES = SMALL + [LARGE]


@pytest.mark.parametrize("F,D,nhid", WIDTHS, ids=["%dx%d" % (d, h) for _, d, h in WIDTHS])
@pytest.mark.parametrize("T,B", F64_CASES, ids=["T%dB%d" % c for c in F64_CASES])
def test_row_block_layer_vs_float64(T, B, F, D, nhid, monkeypatch):
    """Assertion 2.  The row-block launches under the default masks against oracle.restatement.encoder_layer evaluated in float64
    on the same fp32 parameters and inputs, split-bf16 mode, dropout off: the LayerNorm-epilogue and LayerNorm-backward-prologue
    kernels meet exact arithmetic here (elsewhere only the fused chains, with these kernels as THEIR reference).
      * y: 5e-5 x 6 absolute (test_encoder_layer_vs_oracle's bound in this mode);
      * linear2.weight, linear2.bias, norm2.weight, norm2.bias -- continuous in the ReLU gates, a flipped gate has h ~ 0 and does
        not move them: 2e-4 of the tensor's max-norm (the bound of the gate-free split-bf16 sub-graph in
        test_attention_core_vs_float64);
      * every other gradient: relative L2 < 2e-2 and max-norm < 0.25 (test_gpu_parity._grad_close: one gate whose pre-activation
        lies within 1e-5 of zero may open on one side only)."""
    from raindrop_amd import _lib
    _force_row_blocks(monkeypatch)
    x, mask, dy, p = _layer_inputs(T, B, D, nhid, seed=T * 31 + B)
    x64 = x.double().requires_grad_(True)
    p64 = {("L." + n): t.double().requires_grad_(True) for n, t in p.items()}
    y_ref = O2.encoder_layer(x64, mask, p64, "L.", 2)
    g_ref = torch.autograd.grad(y_ref, [x64] + [p64["L." + n] for n in ENC_NAMES], dy.double())
    shp = _lib.shape(B, T, F, 4, nhead=2, nhid=nhid)
    with _rowgemm_stamps() as st:
        y, g = _run_layer(*_to_dev(x, mask, dy, p), shp, 0.0)
        assert st.take().any(), "no k_rowgemm launch"
    ey = float(np.abs(y - y_ref.detach().numpy()).max())
    figures = ["y %.2e" % ey]
    bad = [] if ey < 5e-5 * 6.0 else [("y", ey)]
    for name, a, r in zip(("x",) + ENC_NAMES, g, g_ref):
        r = r.numpy()
        e, e2 = _rel(a, r), _rel2(a, r)
        figures.append("%s %.2e/%.2e" % (name, e, e2))
        if not (e < 2e-4 if name in GATE_FREE else (e2 < 2e-2 and e < 0.25)):
            bad.append((name, e, e2))
    print("float64 tie T=%d B=%d %dx%d (max-norm / L2): %s" % (T, B, D, nhid, ", ".join(figures)))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------------------
# the fused row-local chains' own variants (rd_encfuse.hip), dropout on
# ------------------------------------------------------------------------------------------------------------------------------------
def _live_blocks(stamps, rows):
    """workgroups of k_enc_post_fwd that found live rows: each writes its clocks at [256 + 2 blockIdx] of the forward half of the
    buffer when it starts (workgroups whose first row lies beyond the `rows` live ones return before that); the grid is
    ceil(M / 32) whatever the block height.  rows <= 16384: at most 512 live workgroups, so the start stamps stay below the end
    stamps, which begin at 256 + 1024 (rd_encfuse.hip post_fwd_body points back here)."""
    assert rows <= 16384
    return int(np.count_nonzero(stamps[256:256 + 1024:2]))


def _pick_rows(rows, ncu):
    """rd_encfuse.hip pick_rt: 48-row blocks when 32-row ones need a second round on `ncu` CUs and 48-row ones do not"""
    return 48 if 32 * ncu < rows <= 48 * ncu else 32


def _bwd_launched(stamps):
    """k_enc_pre_bwd: the phase stamps of workgroup 0's waves, at the start of the backward half"""
    return bool(stamps[4096:4096 + 256].any())


# B = 6: 360 rows; 150 / 137: 9000 / 8220 rows, 48-row blocks on a 256-CU device; 256: two rounds of 32-row blocks
CHAIN_CASES = [(60, 6, 34), (60, 150, 34), (60, 256, 34), (60, 6, 36), (60, 137, 36), (60, 256, 36)]


@pytest.mark.parametrize("mode", [1, 2], ids=["bf16x3", "bf16"])
@pytest.mark.parametrize("T,B,F", CHAIN_CASES)
def test_specialised_chains_equal_the_runtime_width_chains(T, B, F, mode, monkeypatch):
    """RD_ENC_SPECIALIZE unset (widths compiled in: k_enc_post_fwd / k_enc_pre_bwd <152, 272> or <160, 288>) against =0 (the <0, 0>
    instantiations reading the widths from their arguments), dropout 0.2: the same code with constants folded -- output and all
    thirteen gradients bit-identical.  Both runs must write the chains' stamps."""
    from raindrop_amd import _lib
    D, nhid = 4 * F + 16, 8 * F
    _lib.call("rd_set_precision", mode)
    x, mask, dy, p = _to_dev(*_layer_inputs(T, B, D, nhid, seed=T * 7 + B))
    shp = _lib.shape(B, T, F, 4, nhead=2, nhid=nhid)
    res = {}
    with _encfuse_stamps() as st:
        for spec in ("default", "0"):
            if spec == "0":
                monkeypatch.setenv("RD_ENC_SPECIALIZE", "0")
            res[spec] = _run_layer(x, mask, dy, p, shp, 0.2)
            s = st.take()
            assert _live_blocks(s, T * B) > 0 and _bwd_launched(s), "RD_ENC_SPECIALIZE %s: chains not launched" % spec
    assert np.array_equal(res["0"][0], res["default"][0]), ("y", _rel(res["0"][0], res["default"][0]))
    for name, a, r in zip(("x",) + ENC_NAMES, res["0"][1], res["default"][1]):
        assert np.array_equal(a, r), (name, _rel(a, r))


@pytest.mark.parametrize("T,B,F", CHAIN_CASES)
def test_chain_block_height_choice_changes_layernorm_partials_only(T, B, F, monkeypatch):
    """RD_ENC_FUSE_TALL=0 (32-row blocks always) against the device's own choice (48-row blocks when 32-row ones need a second round
    and 48-row ones do not: rd_encfuse.hip pick_rt), dropout 0.2.  A row's arithmetic does not depend on its block: everything
    bit-identical except the four LayerNorm affine gradients, whose per-block partials group 32 or 48 rows -- 2e-5 of max-norm.
    The number of forward workgroups that found live rows (stamps) must be ceil(M / 32) with the switch and ceil(M / block height)
    without."""
    from raindrop_amd import _lib
    D, nhid = 4 * F + 16, 8 * F
    M = T * B
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    rows = _pick_rows(M, ncu)
    x, mask, dy, p = _to_dev(*_layer_inputs(T, B, D, nhid, seed=T * 7 + B))
    shp = _lib.shape(B, T, F, 4, nhead=2, nhid=nhid)
    res = {}
    with _encfuse_stamps() as st:
        for tall, want in (("default", rows), ("0", 32)):
            if tall == "0":
                monkeypatch.setenv("RD_ENC_FUSE_TALL", "0")
            res[tall] = _run_layer(x, mask, dy, p, shp, 0.2)
            s = st.take()
            assert _bwd_launched(s), tall
            assert _live_blocks(s, M) == (M + want - 1) // want, (tall, _live_blocks(s, M), M, want)
    assert np.array_equal(res["0"][0], res["default"][0]), ("y", _rel(res["0"][0], res["default"][0]))
    for name, a, r in zip(("x",) + ENC_NAMES, res["0"][1], res["default"][1]):
        if name in LN_AFFINE:
            assert _rel(a, r) <= 2e-5, (name, _rel(a, r))
        else:
            assert np.array_equal(a, r), (name, _rel(a, r))


POISON = 0x7FC07FC0                                  # fp32 NaN = a pair of bf16 NaNs


def _plan_step(cfg, gs, batch, p_drop=0.2):
    """One eager training step on the token plan (the configuration in which the chains run LEAN: rd_temporal.hip enc_route `lean`), run
    twice with the saved buffers of the encoder layers filled with a NaN pattern in between -> (loss, logits, gradients) of the
    second run and the number of 32-bit words of those buffers the second run did not write."""
    from raindrop_amd import dp
    from tests.helpers import build_ours
    dv = {k: (None if v is None else v.to(DEV).clone()) for k, v in batch.items()}
    m = build_ours(cfg, gs, DEV, 7).train()
    m.dropout.p = p_drop
    live = synth.live_parameter_names(cfg)
    named = dict(m.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in live])
    step = TrainStep(m, flat, dv, use_graph=False, token_plan=True, autotune=False)
    try:
        assert step.plan is not None
        words = [t.view(torch.uint8).reshape(-1)[: t.numel() * t.element_size() // 4 * 4].view(torch.int32) for t in step.enc_saved]
        for k in range(2):
            for w in words:
                w.fill_(POISON)
            step.seed_cell.fill_(5)                                      # the step bumps it: same masks in every run
            step.run()
            torch.cuda.synchronize()
        untouched = sum(int((w == POISON).sum()) for w in words)
        mlive = int(step.plan[0])
        return (float(step.loss), step.logits.cpu().numpy().copy(), {n: named[n].grad.detach().cpu().numpy().copy() for n in live},
                untouched, mlive, len(words))
    finally:
        step.close()




# On the token plan the chains see M_live = the sum of the lengths, not T B, and choose their block height from that (pick_rt).  The
# batches are therefore sized by their LIVE rows on the 256 CUs of the device the heights are tuned for (synth.make_batch, seeds
# 23 and 29; `min_len` raises the mean length):
#   (config, B, min_len, body): "one"  = 32-row blocks, a single partial round;
#                               "tall" = M_live in (8192, 12288]: the 48-row bodies post_fwd_body<3> / pre_bwd_body<3>;
#                               "two"  = M_live in (12288, 16384]: 32-row blocks again, two rounds.
# P19 B = 150 / 256 at full length are the sizes of the eager tests above (9000 / 15360 rows); the others are ragged
# (8807 / 8946, 13241 / 13296 and, P12, 8916 / 9260 live rows).
PLAN_CASES = [("P19", 6, 2, "one"), ("P19", 150, 60, "tall"), ("P19", 200, 30, "tall"), ("P19", 256, 60, "two"),
              ("P19", 256, 44, "two"), ("P12", 6, 2, "one"), ("P12", 56, 120, "tall")]
PLAN_IDS = ["%s-B%d-min%d-%s" % c for c in PLAN_CASES]


def _assert_body(stamps, mlive, body, tag):
    """The forward chain's start stamps count the workgroups that found live rows: ceil(M_live / block height), and the height and
    the number of rounds must be those the case was built for."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    rows = _pick_rows(mlive, ncu)
    blocks = (mlive + rows - 1) // rows
    want = {"one": rows == 32 and blocks <= ncu, "tall": rows == 48, "two": rows == 32 and blocks > ncu}[body]
    assert want, "%s: %d live rows on %d CUs do not run the '%s' body this case is sized for" % (tag, mlive, ncu, body)
    assert _bwd_launched(stamps), tag + ": backward chain not launched"
    assert _live_blocks(stamps, mlive) == blocks, (tag, _live_blocks(stamps, mlive), mlive, rows)


@pytest.mark.parametrize("mode", [1, 2], ids=["bf16x3", "bf16"])
@pytest.mark.parametrize("cfg_name,B,min_len,body", PLAN_CASES, ids=PLAN_IDS)
def test_lean_chains_equal_the_chains_with_saved_hidden(cfg_name, B, min_len, body, mode, monkeypatch):
    """RD_ENC_LEAN=0 (the forward chain saves the fp32 FFN hidden h and x1) against the default on the token plan (gate bytes + x1
    re-normalised from the saved pre-norm sum and statistics), whole training step, dropout 0.2, in both bf16 modes (the
    <.., LEAN, ONE> instantiations are the single-product ones): the backward consumes h only as h > 0 and x1 only as the value the
    forward computed from the same sum and statistics -- loss, logits and every gradient bit-identical.
    Non-vacuity: in both runs the forward chain's stamps count ceil(M_live / height) workgroups of the height and round count the
    case names (_assert_body), and the LEAN run leaves at least M_live nhid / 2 more words of the layers' saved buffers unwritten
    (h is M nhid floats, its gate bytes a sixteenth of that)."""
    from raindrop_amd import _lib
    cfg = synth.make_config(cfg_name)
    gs = synth.make_structure(cfg, "sparse")
    batch = synth.make_batch(cfg, B, seed=23, min_len=min_len)
    _lib.call("rd_set_precision", mode)
    res = {}
    with _encfuse_stamps() as st:
        for lean in ("default", "0"):
            if lean == "0":
                monkeypatch.setenv("RD_ENC_LEAN", "0")
            res[lean] = _plan_step(cfg, gs, batch)
            _assert_body(st.take(), res[lean][4], body, "RD_ENC_LEAN " + lean)
    (l1, g1, gr1, free1, mlive, nl), (l0, g0, gr0, free0, _, _) = res["default"], res["0"]
    print("LEAN %s B=%d: M_live %d, unwritten words %d (lean) / %d (RD_ENC_LEAN=0)" % (cfg_name, B, mlive, free1, free0))
    assert mlive == int(batch["lengths"].clamp(0, cfg["max_len"]).sum())
    assert free1 - free0 >= nl * mlive * cfg["nhid"] // 2, (free1, free0, mlive)
    assert np.isfinite(l1) and l1 == l0, (l1, l0)
    assert np.array_equal(g1, g0), _rel(g1, g0)
    for n in gr1:
        assert np.array_equal(gr1[n], gr0[n]), (n, _rel(gr1[n], gr0[n]))


@pytest.mark.parametrize("mode", [1, 2], ids=["bf16x3", "bf16"])
@pytest.mark.parametrize("cfg_name,B,min_len,body", PLAN_CASES, ids=PLAN_IDS)
def test_lean_specialised_chains_equal_the_lean_runtime_width_chains(cfg_name, B, min_len, body, mode, monkeypatch):
    """The LEAN instantiations (token plan) of the chains, widths compiled in against RD_ENC_SPECIALIZE=0, whole training step with
    dropout 0.2, both bf16 modes, at every block height and round count of PLAN_CASES (stamps: _assert_body): loss, logits and
    every gradient bit-identical (the eager layer above runs the non-LEAN instantiations only)."""
    from raindrop_amd import _lib
    cfg = synth.make_config(cfg_name)
    gs = synth.make_structure(cfg, "sparse")
    batch = synth.make_batch(cfg, B, seed=29, min_len=min_len)
    _lib.call("rd_set_precision", mode)
    res = {}
    with _encfuse_stamps() as st:
        for spec in ("default", "0"):
            if spec == "0":
                monkeypatch.setenv("RD_ENC_SPECIALIZE", "0")
            res[spec] = _plan_step(cfg, gs, batch)
            _assert_body(st.take(), res[spec][4], body, "RD_ENC_SPECIALIZE " + spec)
    (l1, g1, gr1, _, _, _), (l0, g0, gr0, _, _, _) = res["default"], res["0"]
    assert np.isfinite(l1) and l1 == l0, (l1, l0)
    assert np.array_equal(g1, g0), _rel(g1, g0)
    for n in gr1:
        assert np.array_equal(gr1[n], gr0[n]), (n, _rel(gr1[n], gr0[n]))
