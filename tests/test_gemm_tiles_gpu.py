"""GPU: the workgroup tiles of the tiled dense product (raindrop_amd/csrc/rd_gemm.hip k_gemm_bf16x3) that no other test selects,
against float64.

dispatch_bf16x3 chooses one of five tiles (64x64, 128x64, 128x128, 64x128, 64x160) by a cost model: a tile bigger than 64x64 needs
at least 2048 workgroups of its own size and next to no padding, which no shape of the rest of the suite reaches -- but an encoder
layer of SYN256 at B = 16 (8192 rows x 2048 / 3120 columns) does.  Each tile is its own instantiation per operand layout, with its
own staging (Stage<KC, 64 / 128 / 160>), LDS size (all four above 48 KB), padded grid, transposing epilogue and row sums.

The operators are called through the C-ABI (rd_linear_fwd, rd_linear_bwd_input, rd_linear_bwd_input_gated, rd_linear_bwd_weight) at
the smallest shapes for which the cost model selects each tile with ragged edges in both dimensions.  Every case

  1. reads the host-side launch log (include/raindrop_hip_debug.h) and asserts the exact set of k_gemm_bf16x3_* names in it: the
     expected tile and no other;
  2. compares with the float64 product of the same fp32 inputs (bias, ReLU, gate; db = column sums of dy) at the bounds
     tests/test_gpu_parity.py holds the 64x64 tile to: forward and input gradient 1e-5 * TOL, dW 2e-5 * TOL, db 2e-5, TOL = 6 in the
     split-bf16 modes and 1 in fp32.  In the one-product bf16 mode the reference is the float64 product of the bf16-rounded
     operands (what the kernel computes, with fp32 accumulation), at 1e-5 * 6;
  3. shows on the reference alone that the bound sees an edge error: the reference without the last reduction index, with its last
     row zeroed and with its last column zeroed each differ from it by more than the bound;
  4. recomputes the last 50 rows and 64 rows around a tile boundary in the middle with a second call on just those rows (for dW:
     columns of dy, which are the rows of that product), which must log a 64x64 name, and compares the two results;
  5. finds the sentinel untouched in the padding columns of the output (where its leading dimension exceeds its width) and in a
     guard behind its last row.

Step 4 asserts EQUALITY for the products (measured bit-equal on the MI355X for every case, and guaranteed by the reduction loop:
an output element is the accumulator of one fixed sequence of v_mfma_f32_16x16x32_bf16 steps -- per 64 k: lo*hi, hi*lo, hi*hi of
k 0..31, then of k 32..63 -- over its own row of A and row of B, whatever the tile, the form of the loop (_npre) or the rows next to
it; the epilogue is per element).  For dW this needs the same reduction slices in both calls, so the second call sets the split-K
target (rd_debug_set_splitk_want) that reproduces the first call's k_per_split.  db is the exception: its row sums are grouped by
the staging (2 threads x 32 k per row on 128-row tiles, 4 x 16 on 64-row ones), a pure change of fp32 summation order, held to 2e-6
of the max-norm.

The arithmetic mode, the launch log and the split-K target are process-wide; each is set inside try / finally and handed back."""
import ctypes
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP32, BF16X3, BF16 = 0, 1, 2
TOL = {FP32: 1.0, BF16X3: 6.0, BF16: 6.0}
MODE_NAME = {FP32: "fp32", BF16X3: "bf16x3", BF16: "bf16"}
FAMILY = "k_gemm_bf16x3_"
SMALL_TILE = {FAMILY + "64x64", FAMILY + "64x64_npre"}
REDUCERS = {"k_reduce_wide", "k_splitk_reduce2"}
SENTINEL = -12345.0
GUARD = 4096                                          # floats behind the last output row
SAME_ARITHMETIC = 2e-6                                # same products, other summation grouping (db only: see the docstring)


def _cdiv(a, b):
    return -(-a // b)


def _lib():
    from raindrop_amd import _lib as L
    return L


def _hooks():
    lib = _lib().load()
    on, read, want = lib.rd_debug_launch_log, lib.rd_debug_launch_log_read, lib.rd_debug_set_splitk_want
    on.argtypes, on.restype = [ctypes.c_int], None
    read.argtypes, read.restype = [ctypes.c_char_p, ctypes.c_size_t], ctypes.c_size_t
    want.argtypes, want.restype = [ctypes.c_int], None
    return on, read, want


@pytest.fixture(autouse=True)
def _process_wide_settings_handed_back():
    """Whatever a case sets -- and whatever an earlier module left set -- the defaults hold before and after each test: split-bf16
    arithmetic, launch log off, split-K target 640 (rd_debug_set_splitk_want(0))."""
    on, _, want = _hooks()
    _lib().call("rd_set_precision", BF16X3)
    want(0)
    try:
        yield
    finally:
        on(0)
        want(0)
        _lib().call("rd_set_precision", BF16X3)


@pytest.fixture(scope="module", autouse=True)
def _hand_back_device_memory():
    """The 17-33 M-element outputs and their float64 references leave large blocks in torch's caching allocator, and
    tests/test_step_launches_gpu.py names buffers by the order in which their addresses first appear: release them here."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _logged(fn):
    """run fn with the launch log on -> the distinct names the launch sites reported"""
    on, read, _ = _hooks()
    buf = ctypes.create_string_buffer(1 << 12)
    on(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        need = read(buf, len(buf))
        on(0)
    assert need < len(buf)
    return {n for n in buf.value.decode().split("\n") if n}


def _tiles(names):
    return {n for n in names if n.startswith(FAMILY)}


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _laid(a, ld=None, offset=0):
    """host [rows, cols] -> device view of the same values with row stride ld, `offset` floats behind a 16-byte boundary; the
    padding columns and everything around the view are NaN: a load the kernel does not mask poisons the output"""
    rows, cols = a.shape
    ld = cols if ld is None else ld
    buf = torch.full((rows * ld + offset + 4,), float("nan"), device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(torch.from_numpy(a))
    assert (view.data_ptr() % 16 == 0) == (offset % 4 == 0) and view.stride() == (ld, 1)
    return view


class _Out:
    """[rows, cols] output with leading dimension ld and GUARD floats behind it, all pre-filled with the sentinel"""

    def __init__(self, rows, cols, ld=None):
        self.rows, self.cols, self.ld = rows, cols, cols if ld is None else ld
        self.buf = torch.full((rows * self.ld + GUARD,), SENTINEL, device=DEV)
        self.full = self.buf[:rows * self.ld].view(rows, self.ld)
        self.t = self.full[:, :cols]

    def assert_nothing_written_outside(self):
        assert bool((self.buf[self.rows * self.ld:] == SENTINEL).all()), "written behind the last row"
        if self.ld > self.cols:
            assert bool((self.full[:, self.cols:] == SENTINEL).all()), "written into the padding columns"
        assert bool(torch.isfinite(self.t).all()) and not bool((self.t == SENTINEL).all(dim=1).any())


def _rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def _operand(t, mode):
    """what the product multiplies, in float64: the fp32 values, or their bf16 roundings in the one-product mode"""
    return t.bfloat16().double() if mode == BF16 else t.double()


def _sees_edge_errors(ref, ref_short, bound, what):
    """Step 3 (a condition on the inputs, on the reference alone): a dropped last reduction index, a zeroed last row and a zeroed
    last column are each errors above the bound."""
    scale = float(ref.abs().max())
    assert float((ref_short - ref).abs().max()) / scale > bound, (what, "last reduction index")
    assert float(ref[-1].abs().max()) / scale > bound, (what, "last row")
    if ref.dim() == 2:
        assert float(ref[:, -1].abs().max()) / scale > bound, (what, "last column")


def _blocks(n, tile_rows):
    """the last 50 rows (ragged by construction) and 64 rows across a tile boundary in the middle, off every alignment"""
    mid = (n // 2) // tile_rows * tile_rows - 27
    assert 0 < mid and mid + 64 < n - 50
    return [(n - 50, n), (mid, mid + 64)]


def _expect_tile(names, tile, mode):
    if mode == FP32:
        assert "k_gemm" in names and not _tiles(names), names
    else:
        assert _tiles(names) == {FAMILY + tile}, (tile, sorted(names))


def _expect_small(names, mode):
    if mode == FP32:
        assert "k_gemm" in names and not _tiles(names), names
    else:
        assert _tiles(names) and _tiles(names) <= SMALL_TILE, sorted(names)


def _report(kind, case, tile, mode, **figures):
    print("gemm-tiles %s %s tile=%s mode=%s " % (kind, case, tile, MODE_NAME[mode]) +
          " ".join("%s=%.3e" % kv for kv in figures.items()), flush=True)


# ---- forward: y[M, N] = act(x[M, K] W[N, K]^T + b), both operands k-contiguous: k_gemm_bf16x3<true, true, ..> ---------------------
# Layouts (a_vec / b_vec of k_gemm_bf16x3: row stride % 4 == 0 and a 16-byte aligned base pointer, per operand):
#   plain   K = 72, ld = 72        a_vec and b_vec: 16-byte loads, one full 64-step plus an 8-wide tail of two whole quads
#   odd     K = 37, ldx = 37       a_vec false (ldx & 3) and b_vec false (W's row stride is K = 37): the scalar k-contiguous loads
#   quad    K = 70, ldx = 72       a_vec: 16-byte loads, the quad at k = 68 masked to two values (its other two are NaN padding);
#                                  b_vec false (W's row stride 70)
#   offset  K = 72, x and W one float behind a 16-byte boundary: a_vec and b_vec false by the pointer test alone
LAYOUTS = {"plain": (72, 72, 0), "odd": (37, 37, 0), "quad": (70, 72, 0), "offset": (72, 72, 1)}       # K, ld of A, pointer offset
#            id                  tile       M     N     layout    act  ldy    mode
FWD = [("128x64",            "128x64",  8189, 2043, "plain",  1, None, BF16X3),
       ("128x128",           "128x128", 8125, 4093, "plain",  0, None, BF16X3),
       ("64x128",            "64x128",  4157, 4093, "plain",  1, None, BF16X3),
       ("64x160-ldy",        "64x160",  4093, 5115, "plain",  0, 5120, BF16X3),      # ldy > N: sentinel in the padding columns
       ("128x64-odd",        "128x64",  8189, 2043, "odd",    0, None, BF16X3),
       ("128x64-quad",       "128x64",  8189, 2043, "quad",   1, None, BF16X3),
       ("128x64-offset",     "128x64",  8189, 2043, "offset", 0, None, BF16X3),
       ("128x64-cols4",      "128x64",  8189, 2044, "plain",  1, None, BF16X3),      # N % 4 == 0: the epilogue's 16-byte stores
       ("128x64-bf16",       "128x64",  8189, 2043, "plain",  0, None, BF16),
       ("128x128-bf16",      "128x128", 8125, 4093, "plain",  1, None, BF16),
       ("64x128-bf16",       "64x128",  4157, 4093, "plain",  0, None, BF16),
       ("64x160-bf16",       "64x160",  4093, 5115, "plain",  1, None, BF16),
       ("128x64-shape-fp32", None,      8189, 2043, "plain",  1, None, FP32)]        # exact fp32: k_gemm, no tile of the family


@pytest.mark.parametrize("case,tile,M,N,layout,act,ldy,mode", FWD, ids=[c[0] for c in FWD])
def test_forward_tile_vs_float64(case, tile, M, N, layout, act, ldy, mode):
    """rd_linear_fwd on the tile the cost model selects for (M, N); the staging path each layout takes is in the table above LAYOUTS
    (a_vec / b_vec).  Steps 1-5 of the module docstring; the row cross-check is an equality."""
    K, ldx, off = LAYOUTS[layout]
    rng = np.random.default_rng(M * 7 + N + K)
    x = _laid(rng.standard_normal((M, K)).astype(np.float32), ldx, off)
    W = _laid((rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32), K, off)
    b = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).to(DEV)
    call = _lib().call
    call("rd_set_precision", mode)

    def run(xs, out):
        return _logged(lambda: call("rd_linear_fwd", xs.shape[0], N, K, _ptr(xs), xs.stride(0), _ptr(W), _ptr(b), _ptr(out.t),
                                    out.ld, act, _stream()))

    y = _Out(M, N, ldy)
    _expect_tile(run(x, y), tile, mode)
    y.assert_nothing_written_outside()

    def ref_of(k):
        r = _operand(x[:, :k], mode) @ _operand(W[:, :k], mode).t() + b.double()
        return torch.relu(r) if act else r

    ref = ref_of(K)
    bound = 1e-5 * TOL[mode]
    err = _rel(y.t, ref)
    _report("fwd", case, tile, mode, err=err, bound=bound)
    _sees_edge_errors(ref, ref_of(K - 1), bound, case)
    assert err < bound, (case, err)
    del ref
    for r0, r1 in _blocks(M, 128):
        sub = _Out(r1 - r0, N)
        _expect_small(run(x[r0:r1], sub), mode)
        sub.assert_nothing_written_outside()
        assert torch.equal(sub.t, y.t[r0:r1]), (case, r0, float((sub.t - y.t[r0:r1]).abs().max()))


# ---- input gradient: dx[M, K_in] = dy[M, N_out] W[N_out, K_in] (gated: where gate > 0), A = dy k-contiguous, B = W row-contiguous:
# k_gemm_bf16x3<true, false, ..>.  The reduction runs over N_out; only A has a vector path (a_vec; the row-contiguous staging is dword
# loads), so the layouts are dy's: plain N_out = 72 / lddy 72; odd 37 / 37; quad 70 / 72; offset 72 behind a misaligned pointer.
# (4093, 5115) selects 64x160 in the forward; here that tile is excluded (no 160-row staging for a row-contiguous B) and the model
# falls back to 128x64.
#             id                 tile       M     K_in  layout    gated  mode
DGRAD = [("128x64",          "128x64",  8189, 2043, "plain",  False, BF16X3),
         ("128x128",         "128x128", 8125, 4093, "plain",  False, BF16X3),
         ("64x128",          "64x128",  4157, 4093, "plain",  False, BF16X3),
         ("no-64x160",       "128x64",  4093, 5115, "plain",  False, BF16X3),
         ("128x64-odd",      "128x64",  8189, 2043, "odd",    False, BF16X3),
         ("128x64-quad",     "128x64",  8189, 2043, "quad",   False, BF16X3),
         ("128x64-offset",   "128x64",  8189, 2043, "offset", False, BF16X3),
         ("128x64-gated",    "128x64",  8189, 2043, "plain",  True,  BF16X3),
         ("128x64-gated-c4", "128x64",  8189, 2044, "plain",  True,  BF16X3),        # K_in % 4 == 0: 16-byte gate reads and stores
         ("64x128-bf16",     "64x128",  4157, 4093, "plain",  False, BF16),          # LO = false on the row-contiguous staging
         ("128x128-gated-bf16", "128x128", 8125, 4093, "plain", True, BF16)]


@pytest.mark.parametrize("case,tile,M,Kin,layout,gated,mode", DGRAD, ids=[c[0] for c in DGRAD])
def test_input_gradient_tile_vs_float64(case, tile, M, Kin, layout, gated, mode):
    """rd_linear_bwd_input / rd_linear_bwd_input_gated on the tile the cost model selects for (M, K_in) with a row-contiguous B; the
    table above DGRAD says which staging each layout reaches.  Steps 1-5; the row cross-check is an equality."""
    Nout, lddy, off = LAYOUTS[layout]
    rng = np.random.default_rng(M * 5 + Kin + Nout)
    dy = _laid(rng.standard_normal((M, Nout)).astype(np.float32), lddy, off)
    W = _laid((rng.standard_normal((Nout, Kin)) / np.sqrt(Nout)).astype(np.float32))
    gate = _laid(rng.standard_normal((M, Kin)).astype(np.float32)) if gated else None
    call = _lib().call
    call("rd_set_precision", mode)

    def run(r0, r1, out):
        d = dy[r0:r1]
        if gated:
            g = gate[r0:r1]
            return _logged(lambda: call("rd_linear_bwd_input_gated", r1 - r0, Nout, Kin, _ptr(d), d.stride(0), _ptr(W), _ptr(g),
                                        g.stride(0), _ptr(out.t), out.ld, _stream()))
        return _logged(lambda: call("rd_linear_bwd_input", r1 - r0, Nout, Kin, _ptr(d), d.stride(0), _ptr(W), _ptr(out.t), out.ld,
                                    _stream()))

    dx = _Out(M, Kin)
    _expect_tile(run(0, M, dx), tile, mode)
    if gated:                                          # a gated-off element is an exact zero, which the output check below allows
        assert bool(torch.isfinite(dx.t).all()) and bool((dx.buf[M * Kin:] == SENTINEL).all())
    else:
        dx.assert_nothing_written_outside()

    def ref_of(n):
        r = _operand(dy[:, :n], mode) @ _operand(W[:n], mode)
        return torch.where(gate > 0, r, torch.zeros_like(r)) if gated else r

    ref = ref_of(Nout)
    bound = 1e-5 * TOL[mode]
    err = _rel(dx.t, ref)
    _report("dgrad", case, tile, mode, err=err, bound=bound)
    _sees_edge_errors(ref, ref_of(Nout - 1), bound, case)
    assert err < bound, (case, err)
    del ref
    for r0, r1 in _blocks(M, 128):
        sub = _Out(r1 - r0, Kin)
        _expect_small(run(r0, r1, sub), mode)
        assert bool((sub.buf[(r1 - r0) * Kin:] == SENTINEL).all())
        assert torch.equal(sub.t, dx.t[r0:r1]), (case, r0, float((sub.t - dx.t[r0:r1]).abs().max()))


# ---- weight gradient: dW[N_out, K_in] = dy[M, N_out]^T x[M, K_in], db = column sums of dy riding on the product as row sums of its
# A operand; both operands row-contiguous: k_gemm_bf16x3<false, false, ..>.  The reduction runs over M.  splitk_plan counts 64x64
# tiles: more than the target (640) of them -> one slice, so the first three run the single-pass row sums on 128- / 64-row staging;
# the last one raises the target to 4096 -> ceil(4096 / 2048) = 2 slices of align64(65) = 128 rows ([0, 128) and [128, 130)): the
# split-K form of a cost-selected tile, the reduce, and the row sums across slices.
#             id               tile       M    N_out K_in  want  slices lddy  ldx   mode
WGRAD = [("128x64",        "128x64",  256, 2043, 8189, 0,    1, None, None, BF16X3),
         ("128x128",       "128x128", 130, 8125, 4093, 0,    1, None, None, BF16X3),
         ("64x128-ld",     "64x128",  200, 4157, 4093, 0,    1, 4160, 4098, BF16X3),     # lddy > N_out, ldx > K_in (NaN padding)
         ("128x64-splitk", "128x64",  130, 2043, 4093, 4096, 2, None, None, BF16X3),
         ("128x64-bf16",   "128x64",  256, 2043, 8189, 0,    1, None, None, BF16)]


def _wgrad(M, Nout, Kin, dy, x, dW, db, want_groups):
    """one rd_linear_bwd_weight call under the split-K target `want_groups` (0: the default, 640) -> (launch names, workspace bytes)"""
    lib = _lib().load()
    _, _, want = _hooks()
    want(want_groups)
    try:
        nbytes = int(lib.rd_linear_bwd_weight_workspace_bytes(M, Nout, Kin))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
        names = _logged(lambda: _lib().call("rd_linear_bwd_weight", M, Nout, Kin, _ptr(dy), dy.stride(0), _ptr(x), x.stride(0),
                                            _ptr(dW.t), _ptr(db.t), _ptr(ws), nbytes, _stream()))
    finally:
        want(0)
    return names, nbytes


@pytest.mark.parametrize("case,tile,M,Nout,Kin,want,slices,lddy,ldx,mode", WGRAD, ids=[c[0] for c in WGRAD])
def test_weight_gradient_tile_vs_float64(case, tile, M, Nout, Kin, want, slices, lddy, ldx, mode):
    """rd_linear_bwd_weight on the tile the cost model selects for (N_out, K_in) and the plan's slice count, with db.  Steps 1-5; the
    workspace size proves the slice count.  Cross-check: a block of dy's columns (rows of the product) in a second call whose
    split-K target reproduces the first call's k_per_split -- dW equal, db within 2e-6 (row sums grouped by the staging's height)."""
    rng = np.random.default_rng(M * 3 + Nout + Kin)
    dy = _laid(rng.standard_normal((M, Nout)).astype(np.float32), lddy)
    x = _laid(rng.standard_normal((M, Kin)).astype(np.float32), ldx)
    _lib().call("rd_set_precision", mode)
    dW, db = _Out(Nout, Kin), _Out(1, Nout)
    names, nbytes = _wgrad(M, Nout, Kin, dy, x, dW, db, want)
    _expect_tile(names, tile, mode)
    assert nbytes == _cdiv(slices * (Nout * Kin + Nout) * 4, 256) * 256                    # wgrad_ws_floats: slices x [dW | db]
    assert bool(names & REDUCERS) == (slices > 1), sorted(names)
    dW.assert_nothing_written_outside()
    db.assert_nothing_written_outside()

    def ref_of(m):
        return _operand(dy[:m], mode).t() @ _operand(x[:m], mode), dy[:m].double().sum(0)

    refW, refb = ref_of(M)
    shortW, shortb = ref_of(M - 1)
    bound = 2e-5 * TOL[mode]
    errW, errb = _rel(dW.t, refW), _rel(db.t[0], refb)
    _report("wgrad", case, tile, mode, err_dW=errW, bound_dW=bound, err_db=errb, bound_db=2e-5)
    _sees_edge_errors(refW, shortW, bound, case + " dW")
    _sees_edge_errors(refb, shortb, 2e-5, case + " db")
    assert errW < bound, (case, errW)
    assert errb < 2e-5, (case, errb)
    del refW, shortW
    worst_db = 0.0
    for c0, c1 in _blocks(Nout, 128):
        n = c1 - c0
        # the target that gives `slices` slices of the same k_per_split on the block's own 64x64 tile count (splitk_plan)
        sub_want = 1 if slices == 1 else slices * _cdiv(n, 64) * _cdiv(Kin, 64)
        sW, sb = _Out(n, Kin), _Out(1, n)
        sub_names, sub_bytes = _wgrad(M, n, Kin, dy[:, c0:c1], x, sW, sb, sub_want)
        _expect_small(sub_names, mode)
        assert sub_bytes == _cdiv(slices * (n * Kin + n) * 4, 256) * 256
        sW.assert_nothing_written_outside()
        assert torch.equal(sW.t, dW.t[c0:c1]), (case, c0, float((sW.t - dW.t[c0:c1]).abs().max()))
        d = float((sb.t[0] - db.t[0, c0:c1]).abs().max() / db.t.abs().max())
        worst_db = max(worst_db, d)
        assert d < SAME_ARITHMETIC, (case, c0, d)
    _report("wgrad-rows", case, tile, mode, db_regrouped=worst_db)
