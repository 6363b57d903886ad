"""GPU: the launches of one encoder layer are exactly those its route names.

rd_debug_encoder_route (include/raindrop_hip_debug.h) reports csrc/rd_temporal.hip's enc_route as a bit mask; one layer forward +
backward (and the inference forward) runs with the launch log on, and the names the launch sites reported must be the set the bits
imply -- the bit-to-names map is `expected` below.  Names of the tiled GEMM family depend on its own tile / grid choices, which are
no business of the route: they are compared by family ("gemm": any k_gemm*; "colsum": k_colsum*; the split-K reduce launches of a
weight gradient are allowed, not required, where the route has the split-K GEMMs).  Every output starts as NaN."""
import ctypes

import pytest
import torch

from raindrop_amd import _lib
from tests.test_rowgemm_variants_gpu import ENC_NAMES, _layer_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAYER, SEED, P_DROP = 1, 77, 0.2
SPLITK = {"k_splitk_reduce", "k_splitk_reduce2", "k_reduce_wide"}
# (T, B, F, nhid, nhead): D = 152 / 272, the row-block kernels and both fused chains; D = 36, the tiled family
ROW_BLOCK, TILED = (13, 5, 34, 272, 2), (7, 3, 5, 40, 2)


def expected(r, T, bf16, infer=False):
    """route fields -> (names that must be logged, names that may be) for one forward + backward, or the inference forward"""
    attn = lambda d: "k_attn_%s_one_b16w" % d if bf16 else {"fwd": "k_attn_fwd", "bwd": "k_attn_bwd_one"}[d]     # T <= 64, head_dim <= 96
    dense = "k_rowgemm" if "rg" in r else "gemm"
    if infer:
        assert "infer" in r
        return {"k_wsplit", "k_enc_post_infer"} | ({"k_attn_fwd_fused<save-free>"} if "afuse_fwd" in r else {"k_rowgemm", attn("fwd")}), set()
    assert T <= 64
    need = {"k_wsplit"} if r & {"rg", "panel"} else set()
    # forward: in_proj + attention core
    need |= {"k_attn_fwd_fused"} if "afuse_fwd" in r else {dense} | ({"gemm", "k_softmax_rows"} if "big" in r else {attn("fwd")})
    # forward: out_proj .. LayerNorm2
    if "chain_fwd" in r:
        need |= {"k_enc_post_fwd"}
    else:
        need |= {dense}                                                                      # linear1
        need |= {"k_rowgemm_ln"} if r & {"lnf1", "lnf2"} else set()
        need |= {dense, "k_add_ln_fwd_v"} if not {"lnf1", "lnf2"} <= r else set()
    # backward: LayerNorm2' .. out_proj'
    if "chain_bwd" in r:
        need |= {"k_enc_pre_bwd"}
    elif "lnb" in r:
        need |= {"k_rowgemm_lnb", "k_rowgemm"}
    else:
        need |= {"k_ln_bwd_v", dense}
    # backward: attention core + in_proj'
    if "afuse_bwd" in r:
        need |= {"k_attn_bwd_fused"}
    else:
        need |= {"gemm", "k_softmax_bwd_rows"} if "big" in r else {attn("bwd")}
        need |= {"k_rowgemm" if "dx_rowblock" in r else "gemm"}
    # weight gradients and the LayerNorm column sums
    wg_gemm = not r & {"tw", "tw2"}
    if "tw" not in r:
        need |= {"colsum"}
    if wg_gemm:
        need |= {"gemm"}
    else:
        need |= {"k_twg", "k_twg_reduce"} | ({"k_rows_to_tiles"} if "tw2" in r else set())
    return need, (SPLITK if wg_gemm else set())


def _family(name):
    return "gemm" if name.startswith("k_gemm") else "colsum" if name.startswith("k_colsum") else name


def _route(shp, plan):
    bits = ctypes.c_uint32(0)
    _lib.call("rd_debug_encoder_route", ctypes.byref(shp), int(plan), ctypes.byref(bits))
    return {n for i, n in enumerate(_lib.ROUTE_BITS) if bits.value >> i & 1}


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _run(dims, mode, plan, infer):
    """-> (route fields, logged names); asserts that everything the calls must write is finite"""
    T, B, F, nhid, nhead = dims
    D = 4 * F + 16
    lib = _lib.load()
    on, read = lib.rd_debug_launch_log, lib.rd_debug_launch_log_read
    on.argtypes, on.restype = [ctypes.c_int], None
    read.argtypes, read.restype = [ctypes.c_char_p, ctypes.c_size_t], ctypes.c_size_t
    shp = _lib.shape(B, T, F, 4, nhead=nhead, nhid=nhid)
    sp = ctypes.byref(shp)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, mask, dy, p = _layer_inputs(T, B, D, nhid, seed=T * 31 + B)
    lengths = (~mask.bool()).sum(1).long()
    mlive = int(lengths.sum()) if plan else T * B                # on a plan x, y, dy, dx hold the live rows only, rows >= M_live unused
    x, dy, mask = x.reshape(T * B, D).to(DEV), dy.reshape(T * B, D).to(DEV), mask.to(DEV)
    params = [p[n].to(DEV).contiguous() for n in ENC_NAMES]
    grads = [_nan(*t.shape) for t in params]
    w, g = _lib.RdEncoderPtrs(*[t.data_ptr() for t in params]), _lib.RdEncoderPtrs(*[t.data_ptr() for t in grads])
    y, dx = _nan(T * B, D), _nan(T * B, D)
    ws = torch.zeros(int(lib.rd_encoder_layer_workspace_bytes(sp)) + 256, dtype=torch.uint8, device=DEV)
    nsaved = lib.rd_encoder_layer_infer_bytes(sp) if infer else lib.rd_encoder_layer_saved_bytes(sp)
    saved = torch.zeros(int(nsaved) + 256, dtype=torch.uint8, device=DEV)
    tp = torch.zeros(max(int(lib.rd_token_plan_bytes(sp)) // 4, 64), dtype=torch.int32, device=DEV)
    buf = ctypes.create_string_buffer(1 << 12)
    _lib.call("rd_set_precision", mode)
    try:
        r = _route(shp, plan)
        if plan:
            _lib.call("rd_token_plan", sp, _P(lengths.to(DEV)), _P(tp), None, 0, st)
            _lib.call("rd_set_token_plan", _P(tp))
        on(1)
        if infer:
            _lib.call("rd_encoder_layer_fwd_infer", sp, LAYER, _P(x), _P(mask), ctypes.byref(w), _P(y), _P(saved), nsaved, _P(ws),
                      ws.numel(), st)
        else:
            _lib.call("rd_encoder_layer_fwd", sp, LAYER, _P(x), _P(mask), ctypes.byref(w), P_DROP, SEED, _P(y), _P(saved), nsaved,
                      _P(ws), ws.numel(), st)
            _lib.call("rd_encoder_layer_bwd", sp, LAYER, _P(x), _P(mask), ctypes.byref(w), P_DROP, SEED, _P(saved), nsaved, _P(dy),
                      _P(dx), ctypes.byref(g), _P(ws), ws.numel(), st)
        torch.cuda.synchronize()
        assert read(buf, len(buf)) < len(buf)
    finally:
        on(0)
        _lib.call("rd_set_token_plan", None)
        _lib.call("rd_set_precision", 1)
    assert bool(torch.isfinite(y[:mlive]).all()), "y"
    if not infer:
        assert bool(torch.isfinite(dx[:mlive]).all()), "dx"
        for n, t in zip(ENC_NAMES, grads):
            assert bool(torch.isfinite(t).all()), n
    return r, {n for n in buf.value.decode().split("\n") if n}


CASES = [(ROW_BLOCK, 1, False, False), (ROW_BLOCK, 1, True, False), (ROW_BLOCK, 1, False, True), (ROW_BLOCK, 1, True, True),
         (ROW_BLOCK, 0, False, False), (TILED, 1, False, False), (TILED, 0, False, False)]


@pytest.mark.parametrize("dims,mode,plan,infer", CASES,
                         ids=["%s-%s-%s%s" % ("D152" if d is ROW_BLOCK else "D36", {0: "fp32", 1: "bf16x3"}[m], "plan" if pl else "padded",
                                              "-infer" if i else "") for d, m, pl, i in CASES])
def test_logged_launches_are_the_route(dims, mode, plan, infer):
    r, names = _run(dims, mode, plan, infer)
    need, may = expected(r, dims[0], mode != 0, infer)
    got = {_family(n) for n in names}
    print(sorted(r), sorted(names))
    assert need <= got and got <= need | may, {"route": sorted(r), "missing": sorted(need - got), "unexpected": sorted(got - need - may)}
    # what the two shapes are here for
    if dims is ROW_BLOCK and mode == 1:
        assert {"rg", "tw", "chain_fwd", "chain_bwd", "infer", "plan_ok"} <= r and (("afuse_fwd" in r) == plan)
    else:
        assert not r & {"rg", "tw", "chain_fwd", "chain_bwd"} and ("panel" in r) == (mode == 1)
