"""Static steps for `Raindrop_v2`: forward + CrossEntropyLoss + backward as ONE hipGraph.

`code/Raindrop.py:319-323` runs `model.forward -> criterion -> loss.backward()` through autograd,
~100 host-side launches per step.  Every stage of this model already has a forward and a backward
entry point in the C-ABI, so the step can be written out explicitly -- no autograd graph, no
Python in the replay path, every buffer allocated once:

    z, mask          <- rd_sensor_stage_fwd                     (K1 + PE + mask)
    x_{l+1}          <- rd_encoder_layer_fwd(x_l)               (K2/K3, per layer)
    feat = [agg|emb] <- rd_masked_mean_fwd, rd_linear_fwd       (K5; both write into one buffer)
    logits           <- rd_linear_fwd x2
    loss, dlogits    <- rd_softmax_xent                         (CrossEntropyLoss fwd+bwd, one launch; rd_softmax_xent_crit
                                                                with class_weight= / label_smoothing=)
    ... the same chain backwards, each gradient written straight into its slice of the flat
    gradient buffer (raindrop_amd.dp.FlatGradAllReduce): no accumulate kernels, no packing copy.

How the host layer is laid out:

* `Step` owns the buffers (`_Arena`), one enqueue method per STAGE (`_begin`, `_sensor_fwd`, `_enc_fwd`, `_head_train`,
  `_head_fwd`, `_head_bwd`, `_enc_bwd_top`, `_enc_bwd_rest`, `_sensor_bwd`) and the table `Step.PARTS`, which says which stages
  make up each part a caller may enqueue or capture.  Every stage enqueues through the per-instance hook `_call`.
* `has_backward` is a constructor-level fact: without it (raindrop_amd/evalstep.py) no gradient table, gradient buffer, backward
  workspace, seed cell or trailing rider exists, and the head runs operator by operator up to the logits.  Such a step runs the
  INFERENCE forward of every stage (`rd_sensor_stage_fwd_infer` / `rd_beta_stage_fwd_infer`, `rd_encoder_layer_fwd_infer`: the same
  z, x and logits bit for bit, nothing written that only a backward reads) on buffers of the `rd_*_infer_bytes` sizes;
  `save_free=False` keeps the training forward and its buffers (A/B, parity tests).
* What differs between the default branch and `use_beta` sits in a sensor-stage object (`SensorStage` here, `BetaSensorStage` in
  raindrop_amd/step_beta.py): model validation, buffer sizes, extra buffers, the forward and the backward call, and whether
  rd_step_prepare's K1 weight tiles apply.
* Which loss entry point a head runs -- plain, `_crit` (class weights / label smoothing) or `_focal` -- and the buffer it takes is
  decided in `criterion_entry`; `Step._loss_entry` applies it to the step's `crit` / `focal` buffers, feed.validate to its own.
* `capture_graphs` is the one place that warms up on a side stream, joins, synchronizes and captures.
* `TrainStep` adds what training needs: the two-graph data-parallel form, the autotune of the row-block knobs, the measurement
  captures of bench.py, `capture_full` with the optimizer inside, and gradient accumulation (`accumulate=k`: every form captured
  twice, the window's accumulate / close launch behind the body).
* `TrainStep._enqueue` is the one statement of a micro-batch's order: feed gather | per part of `_parts()` the body, the window's
  launch and the caller's `after_part` | (capture_full: the optimizer) | feed record.  Every form is that method with other
  arguments: the eager `run()`, the per-graph bodies of `_capture_one`, `capture_full`'s graphs, and `_warm`, the warm-up all
  captures share.  `_collectives` is the gradient all-reduce as an `after_part`, for `run_allreduce` and `capture_full` alike.

The captured graph is replayed per step; dropout masks change per replay through the device seed
cell (`rd_set_seed_cell` / `rd_seed_cell_advance`), which the graph bumps itself.  The gradient
all-reduce (N > 1) and the Adam kernel stay outside the graph.  The eager model (`models_rd.py`)
and this step call the SAME kernels in the same order; `tests/test_gpu_parity.py` checks that the
gradients agree bit for bit, `tests/test_step_launches_gpu.py` that every form enqueues what it always did.
"""
import contextlib
import ctypes
import gc
import os
import time

import torch

from . import _lib, ops


@contextlib.contextmanager
def _graph_capture(graph, **kw):
    """torch.cuda.graph with Python's cyclic garbage collector held off for the capture.  A model and its captured steps refer to each
    other (Raindrop_v2._graph_runners -> TrainStep -> model), so an unreachable one is freed by the collector, at whatever point an
    allocation triggers it; inside another capture that would destroy its hipGraphs while a capture is in progress, which the
    runtime refuses (the process aborts).  The garbage is collected after the capture instead."""
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, **kw):
            yield
    finally:
        if was_enabled:
            gc.enable()


def warm_up(enqueue, passes=2, no_grad=True):
    """`enqueue()` `passes` times on a side stream (lazy initialisations happen here, not in a capture), joined and synchronized."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), (torch.no_grad() if no_grad else contextlib.nullcontext()):
        for _ in range(passes):
            enqueue()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def capture_graphs(bodies, warm=None):
    """One hipGraph per callable of `bodies`, captured in order out of one memory pool, after two warm-up passes of `warm`
    (default: the bodies in order).  Replaying the graphs in order is what the bodies enqueue."""
    def all_bodies():
        for body in bodies:
            body()
    warm_up(warm or all_bodies)
    graphs = []
    for body in bodies:
        g = torch.cuda.CUDAGraph()
        with torch.no_grad(), _graph_capture(g, **({"pool": graphs[-1].pool()} if graphs else {})):
            body()
        graphs.append(g)
    return graphs


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def plan_supported(d_inp, d_ob, T, D, nhead, nhid, precision):
    """Shapes / modes whose whole step runs on kernels that read a token plan (include/raindrop_hip.h "token plan"): a bf16
    arithmetic mode (precision 1 = bf16x3, 2 = bf16), the fused row-local encoder chains (ceil(D / 32) == 5 and
    ceil(nhid / 32) == 9: the P19 and P12 widths), head_dim <= 96 (single-tile attention for T <= 64 -- with in_proj fused in,
    rd_attnfuse.hip -- or the multi-tile kernels beyond), and either message-passing form (fused LDS-resident for F <= 48,
    K <= 240 in bf16x3, else the panel products whose last scatter follows the plan).  Round 3 had this for the P19 envelope
    only; P12 (T = 215) joined in round 4.  The usual A/B switches of the kernels it relies on turn it off."""
    hd = D // nhead
    env_on = all(os.environ.get(k, "1") != "0" for k in ("RD_ROWGEMM", "RD_TILE_WGRAD", "RD_ATTN_B16", "RD_ATTN_B16_MT", "RD_LN_FUSE",
                                                         "RD_LNB_FUSE", "RD_ENC_FUSE", "RD_HEAD_FUSED"))
    return (precision in (1, 2) and d_ob == 4 and hd * nhead == D and hd <= 96 and (D + 31) // 32 == 5 and (nhid + 31) // 32 == 9
            and D % 4 == 0 and nhid % 4 == 0 and env_on and os.environ.get("RD_ATTN_BIG", "0") == "0")


def validate_batch(model, batch, labels=True):
    """The step hands raw data_ptr()s to the C-ABI: everything the autograd wrappers check per call is checked here
    once (dtype, contiguity, device, shapes, label range).  Labels are read on the host ONCE, at construction."""
    T, B = batch["src"].shape[0], batch["src"].shape[1]
    want = {"src": (torch.float32, (T, B, 2 * model.d_inp)), "times": (torch.float32, (T, B)),
            "lengths": (torch.int64, (B,))}
    if labels:
        want["y"] = (torch.int64, (B,))
    if model.static:
        want["static"] = (torch.float32, (B, model.d_static))
    dev = batch["src"].device
    for k, (dt, shape) in want.items():
        t = batch.get(k)
        if t is None or not t.is_cuda or t.device != dev:
            raise _lib.RaindropHipError("TrainStep: batch[%r] must be a tensor on %s" % (k, dev))
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.RaindropHipError("TrainStep: batch[%r] must be contiguous %s %s, got %s %s" % (
                k, dt, shape, t.dtype, tuple(t.shape)))
    if T != model.max_len:
        raise _lib.RaindropHipError("TrainStep: src.shape[0] (%d) must equal max_len (%d)" % (T, model.max_len))
    if B > 0 and labels:
        lo, hi = int(batch["y"].min()), int(batch["y"].max())
        if lo < 0 or hi >= model.n_classes:
            raise _lib.RaindropHipError("TrainStep: labels must lie in [0, %d), got [%d, %d]" % (model.n_classes, lo, hi))


def criterion_values(class_weight, label_smoothing, n_classes):
    """The device criterion buffer's contents `[eps, w_0 .. w_{C-1}]` (include/raindrop_hip.h rd_softmax_xent_crit) for
    `torch.nn.CrossEntropyLoss(weight=class_weight, label_smoothing=label_smoothing)`, or None for that criterion's defaults
    (`class_weight=None` and `label_smoothing=0`: the plain mean cross entropy, which needs no buffer).  `class_weight`: a sequence
    or 1-d tensor of `n_classes` finite values >= 0 (as fp32); `label_smoothing` in [0, 1).  Anything else: ValueError."""
    eps = float(label_smoothing)
    if not 0.0 <= eps < 1.0:                                       # NaN fails both comparisons
        raise ValueError("label_smoothing must lie in [0, 1), got %r" % (label_smoothing,))
    if class_weight is None:
        if eps == 0.0:
            return None
        return [eps] + [1.0] * int(n_classes)
    w = torch.as_tensor(class_weight.detach().cpu() if isinstance(class_weight, torch.Tensor) else list(class_weight),
                        dtype=torch.float64)
    if w.dim() != 1 or w.numel() != int(n_classes):
        raise ValueError("class_weight must hold n_classes = %d values, got shape %s" % (n_classes, tuple(w.shape)))
    w32 = w.to(torch.float32)
    if not bool(torch.isfinite(w32).all()) or bool((w32 < 0).any()):
        raise ValueError("class_weight must be finite and >= 0, got %s" % (w.tolist(),))
    return [eps] + [float(v) for v in w32.tolist()]


FOCAL_GAMMA_MAX = 16.0


def focal_values(class_weight, focal_gamma, n_classes):
    """The device buffer `[gamma, w_0 .. w_{C-1}]` of the focal loss (include/raindrop_hip.h rd_softmax_xent_focal):
    loss = sum_b w[y_b] q_b^gamma (-log p[b,y_b]) / sum_b w[y_b], q_b the summed probability of the other classes.  `focal_gamma`: a
    finite number in [0, 16] (0: CrossEntropyLoss(weight=class_weight) through the focal kernels); `class_weight` as in
    `criterion_values` (None: all 1).  Anything else: ValueError."""
    if focal_gamma is None or isinstance(focal_gamma, (bool, str, bytes)):
        raise ValueError("focal_gamma must be a finite number in [0, %g], got %r" % (FOCAL_GAMMA_MAX, focal_gamma))
    try:
        gamma = float(focal_gamma)
    except (TypeError, ValueError):
        raise ValueError("focal_gamma must be a finite number in [0, %g], got %r" % (FOCAL_GAMMA_MAX, focal_gamma)) from None
    if not 0.0 <= gamma <= FOCAL_GAMMA_MAX:                        # NaN and the infinities fail
        raise ValueError("focal_gamma must be a finite number in [0, %g], got %r" % (FOCAL_GAMMA_MAX, focal_gamma))
    w = criterion_values(class_weight, 0.0, n_classes)
    return [gamma] + ([1.0] * int(n_classes) if w is None else w[1:])


def criterion_entry(focal, crit):
    """(suffix, buffer): which instantiation of a loss entry point runs (`rd_head_train` / `rd_softmax_xent` + suffix) and the buffer
    it takes behind `y` -- the focal loss's, else the weighted / smoothed criterion's, else ("", None): the plain mean cross entropy,
    whose entry points take no buffer.  The one place that makes this choice (the steps' heads, feed.validate)."""
    return ("_focal", focal) if focal is not None else ("_crit", crit) if crit is not None else ("", None)


def _spliced(buf):
    """the argument a criterion buffer adds to a call: none without one"""
    return () if buf is None else (_p(buf),)


def check_focal(label_smoothing, focal_gamma):
    """focal_gamma together with label smoothing has no agreed meaning: refused (ValueError)."""
    if focal_gamma is not None and float(label_smoothing) != 0.0:
        raise ValueError("label_smoothing=%r together with focal_gamma=%r is refused: smoothed targets have no agreed meaning under "
                         "a focal factor" % (label_smoothing, focal_gamma))


class SensorStage:
    """The sensor stage of the DEFAULT branch (rd_sensor_stage_fwd / rd_msgpass_bwd: code/models_rd.py:317's `use_beta = False`,
    distance exactly 0), and the interface a step asks its sensor stage through.
    Coefficient dropout: `coef_p` = (p1, p2), the model's `ob_propagation.dropout` / `ob_propagation_layer2.dropout` read when the step
    is built (raindrop_amd.models_rd.coef_dropout_of: training-mode model; only a step with a backward -- an evaluation step never
    drops).  With one of them non-zero the forward stage starts with the table launch (rd_msgpass_coef_table into `step.k1_coef`
    [2,B,F], sample b = the caller's batch index with or without a token plan) and both directions run the `_coef` entry points;
    with both zero the stage enqueues exactly what it always did.  The masks follow the step's seed and seed cell like the model's
    own dropout: fresh per replay, the rank offset in the data-parallel form."""
    prepared_tiles = True         # rd_step_prepare's K1 weight tiles are this stage's
    distance = None
    coef_p = (0.0, 0.0)

    @property
    def edge_drop(self):
        """the step draws coefficient-dropout masks: its seed cell must advance per replay even with the model's dropout at 0"""
        return self.coef_p[0] > 0.0 or self.coef_p[1] > 0.0

    def check(self, model):
        """A model built with the paper's branch switched on would silently train a different network here (and never see
        gradients for increase_dim / map_weights): refuse it."""
        if getattr(model, "use_beta", False) or getattr(model, "compute_distance", False):
            raise _lib.RaindropHipError("TrainStep: Raindrop_v2(use_beta=True / compute_distance=True) runs on the eager model "
                                        "surface only (model.forward + autograd); the captured step implements the default branch")

    def buffer_bytes(self, step):
        """(saved, workspace) bytes: the sizes of step.k1_saved / step.k1_ws (rd_msgpass_workspace_bytes is the backward's)"""
        if step.infer:                                            # the weight tiles alone where rd_infer_covers says 1
            return int(step.lib.rd_msgpass_infer_bytes(step.sp)), 0
        return (int(step.lib.rd_msgpass_saved_bytes(step.sp)),
                int(step.lib.rd_msgpass_workspace_bytes(step.sp)) if step.has_backward else 0)

    def alloc(self, step):
        from .models_rd import coef_dropout_of
        self.coef_p = coef_dropout_of(step.model) if step.has_backward else (0.0, 0.0)
        if self.edge_drop:
            g = step.graph_info
            self.ei, self.ew = g["edge_index"].contiguous(), g["edge_weights"].contiguous()   # [2,E] int64 (rows E apart), [E]
            ops._validate_edges(self.ei, step.model.d_inp, "TrainStep")
            step.k1_coef = torch.zeros((2, step.B, step.model.d_inp), dtype=torch.float32, device=step.dev)

    def _weights(self, P):
        return [P["ob_propagation" + n] for n in (".lin_value.weight", ".lin_value.bias", "_layer2.lin_value.weight", "_layer2.lin_value.bias")]

    def forward(self, s, st):
        b, P = s.batch, s.P
        W1, b1, W2, b2 = self._weights(P)
        if s.infer:
            return s._call("rd_sensor_stage_fwd_infer", s.sp, _p(b["src"]), _p(b["times"]), _p(b["lengths"]), _p(s.ts), _p(P["R_u"]),
                           _p(W1), _p(b1), _p(W2), _p(b2), _p(s.graph_info["ssum"]), _p(s.z), _p(s.mask), _p(s.k1_saved),
                           s.k1_saved.numel(), 1 if s.prep_k1 else 0, st)
        coef = ()
        if self.edge_drop:                                        # this replay's coefficient table, under the step's seed + seed cell
            s._call("rd_msgpass_coef_table", s.B, s.model.d_inp, int(self.ei.shape[1]), _p(self.ei), self.ei.stride(0), _p(self.ew),
                    _p(s.graph_info["ssum"]), self.coef_p[0], self.coef_p[1], s.seed, _p(s.k1_coef), st)
            coef = (_p(s.k1_coef),)
        s._call(("rd_sensor_stage_fwd_prepared" if s.prep_k1 else "rd_sensor_stage_fwd") + ("_coef" if coef else ""), s.sp,
                _p(b["src"]), _p(b["times"]), _p(b["lengths"]), _p(s.ts), _p(P["R_u"]), _p(W1), _p(b1), _p(W2), _p(b2),
                _p(s.graph_info["ssum"]), *coef, s.p_drop, s.seed, _p(s.z), _p(s.mask), _p(s.k1_saved), s.k1_saved.numel(), st)

    def backward(self, s, cur, st):
        b, P = s.batch, s.P
        W1, _, W2, _ = self._weights(P)
        coef = (_p(s.k1_coef),) if self.edge_drop else ()
        s._call("rd_msgpass_bwd_coef" if coef else "rd_msgpass_bwd", s.sp, _p(b["src"]), _p(P["R_u"]), _p(W1), _p(W2),
                _p(s.graph_info["ssum"]), *coef, s.p_drop, _p(s.k1_saved), s.k1_saved.numel(), _p(s.z), _p(cur), s.D, *[_p(g) for g in self._weights(s.G)], _p(s.G["R_u"]),
                _p(s.k1_ws), s.k1_ws.numel(), st)


class _Arena:
    """Every buffer of a step carved out of ONE zero-filled allocation (round 6; RD_STEP_ARENA=0: separate torch allocations, A/B):
    the large ones on 2-MB boundaries, the small ones (< 1 MB: head workspace, features, plan, ...) packed at 256-byte
    granularity into a common 16-MB region in front.  Why: the K1 backward kernel's duration was bimodal BETWEEN PROCESSES (16.4
    vs 18.6 us, HISTORY round 5: "it follows how the process's memory is mapped") -- with one contiguous mapping it is
    16.2-16.6 us in every process and the step's kernel sum drops 0.6 % (four processes each, alternating, one call:
    profiles/r06_step_arena_ab.txt).  Every kernel of a step starts on cold translations (~1 GB of traffic since its last run);
    fewer, larger mappings are fewer walks.  `large`: the byte counts of the large buffers, known up front; a buffer the list
    missed gets an allocation of its own.  Zero-filled: with a token plan parts of these buffers are never written, and a ghost
    product (x 0) of an uninitialised NaN pattern would not be 0."""

    def __init__(self, dev, large):
        self.dev, self.buf = dev, None
        if os.environ.get("RD_STEP_ARENA", "1") == "1":
            small_cap = 16 << 20
            self.buf = torch.zeros(sum(self.al(n) for n in large) + small_cap + (1 << 21), dtype=torch.uint8, device=dev)
            self.small = (-self.buf.data_ptr()) % (1 << 21)
            self.small_end = self.off = self.small + small_cap

    @staticmethod
    def al(n):
        return (max(int(n), 256) + (1 << 21) - 1) >> 21 << 21

    def u8(self, nbytes):
        n = max(int(nbytes), 256)
        if self.buf is not None:
            if n < (1 << 20) and self.small + n <= self.small_end:
                o = self.small
                self.small += (n + 255) >> 8 << 8
                return self.buf[o:o + n]
            o = self.off
            self.off += self.al(n)
            if self.off <= self.buf.numel():
                return self.buf[o:o + n]
        return torch.zeros(n, dtype=torch.uint8, device=self.dev)

    def zeros(self, shape):
        if self.buf is None:
            return torch.zeros(shape, dtype=torch.float32, device=self.dev)
        n = int(torch.Size(shape).numel()) * 4
        return self.u8(n)[:n].view(torch.float32).view(shape)


class Step:
    """Buffers, stages and parts of a captured step; `TrainStep` and `EvalStep` (raindrop_amd/evalstep.py) are built on it."""
    # part -> the stages it enqueues, in order.  None: the whole training step; 'a' / 'b': the two halves of the data-parallel
    # form (TrainStep.__init__); 'begin' / 'k1f' / 'mid' / 'k1b': the step cut around the message-passing stage, 'enc' / 'head' /
    # 'encb': 'mid' cut further (capture_segments / capture_marked: bench.py times the K1 launches and the encoder layers as they
    # run INSIDE the step); 'mf' / 'mb': forward up to the logits and backward from `dlogits` (graph_module; EvalStep runs 'mf')
    PARTS = {
        None:    ("begin", "sensor_fwd", "enc_fwd", "head_train", "enc_bwd_top", "enc_bwd_rest", "sensor_bwd"),
        "a":     ("begin", "sensor_fwd", "enc_fwd", "head_train", "enc_bwd_top"),
        "b":     ("enc_bwd_rest", "sensor_bwd"),
        "begin": ("begin",),
        "k1f":   ("sensor_fwd",),
        "mid":   ("enc_fwd", "head_train", "enc_bwd_top", "enc_bwd_rest"),
        "enc":   ("enc_fwd",),
        "head":  ("head_train",),
        "encb":  ("enc_bwd_top", "enc_bwd_rest"),
        "k1b":   ("sensor_bwd",),
        "mf":    ("begin", "sensor_fwd", "enc_fwd", "head_fwd"),
        "mb":    ("head_bwd", "enc_bwd_top", "enc_bwd_rest", "sensor_bwd"),
    }

    def __init__(self, model, batch, sensor, flat=None, has_backward=True, labels=True, p_drop=None, seed=1234, token_plan=None,
                 save_free=True, class_weight=None, label_smoothing=0.0, focal_gamma=None):
        """sensor: the sensor-stage object of the model's branch.  has_backward=False: a forward-only step -- no gradient tables,
        no dx / dfeat / dhid / dlogits / loss / weight-gradient workspace, no backward workspaces, seed cell or trailing riders,
        dropout off whatever model.training says, the eager surface's head operator by operator, and (save_free, the default) the
        inference forward of every stage on buffers of the inference sizes.  save_free has no meaning with a backward.
        class_weight / label_smoothing: the step's loss is torch.nn.CrossEntropyLoss(weight=class_weight,
        label_smoothing=label_smoothing) (mean reduction; `criterion_values` has the accepted values, ValueError otherwise) --
        the step then owns a device buffer `crit` = [eps, w_0 ..] and its head runs the `_crit` entry points (rd_head_train_crit /
        rd_softmax_xent_crit), which read that buffer when they RUN: `set_criterion` changes both between replays.  The mean's
        denominator is the sum of w[y_b] over THIS step's batch: under data parallelism every rank normalises by its own shard
        and the gradient all-reduce averages the ranks, which is what DistributedDataParallel with torch's criterion computes.
        Both at their defaults: the plain mean cross entropy, no buffer, the launches the step always enqueued.
        focal_gamma: a number in [0, 16] (0.0 included) makes the loss the focal loss with these class weights (`focal_values`;
        label_smoothing must be 0): the step owns `focal` = [gamma, w_0 ..] instead of `crit` and its head runs the `_focal` entry
        points (rd_head_train_focal / rd_softmax_xent_focal) on it; `set_criterion(class_weight=, focal_gamma=)` changes both
        between replays.  The denominator and the data-parallel rule are the weighted criterion's.  None: as without it."""
        crit, focal = criterion_values(class_weight, label_smoothing, model.n_classes), None
        check_focal(label_smoothing, focal_gamma)
        if focal_gamma is not None:
            crit, focal = None, focal_values(class_weight, focal_gamma, model.n_classes)
        if (crit is not None or focal is not None) and not (has_backward and labels):
            raise ValueError("class_weight / label_smoothing / focal_gamma belong to a step that evaluates the loss itself (a training step with labels)")
        self.model, self.flat, self.batch, self.sensor, self.has_backward = model, flat, batch, sensor, bool(has_backward)
        self.infer = bool(save_free) and not self.has_backward
        self.dev = batch["src"].device
        self.lib = _lib.load()
        cfgp = float(model.dropout.p) if p_drop is None else float(p_drop)
        self.p_drop = cfgp if model.training and has_backward else 0.0
        self.seed = (int(seed) + ops.rank_seed_offset()) & 0x7FFFFFFFFFFFFFFF if has_backward else 0   # ranks draw different dropout masks
        sensor.check(model)
        validate_batch(model, batch, labels=labels)
        T, B = batch["src"].shape[0], batch["src"].shape[1]
        self.T, self.B = T, B
        self.shp = _lib.shape(B, T, model.d_inp, model.d_ob, d_pe=model.d_pe, nhead=model.nhead, nhid=model.nhid,
                              d_static=model.d_static if model.static else 0, n_classes=model.n_classes,
                              max_len=model.max_len)
        self.sp = ctypes.byref(self.shp)
        self.D = model.d_inp * model.d_ob + model.d_pe
        self.graph_info = model._graph(self.dev)                 # adjacency / ssum (built eagerly, once)
        self.ts = model.pos_encoder.timescales(self.dev)
        self.P = dict(model.named_parameters())
        self.G = dict(zip(flat.names, flat.views)) if has_backward else {}      # gradient slices in the flat buffer
        self._alloc(crit, focal)
        self.seed_cell = torch.zeros(1, dtype=torch.int64, device=self.dev) if has_backward else None
        # side branch for the trailing launches of the step (the weight-gradient reduces, the head's weight gradients: nothing in
        # the backward chain reads them).  MEASURED round 4, same box, 3 x 300 steps each: 0.554 ms/step with the branch against
        # 0.521 without -- the fourth time a forked graph loses here (the fork / join edges cost more than the 5-8 us launches
        # they take off the chain).  Off by default; RD_SIDE_REDUCE=1 turns it on (results are identical).
        side = has_backward and os.environ.get("RD_SIDE_REDUCE", "0") == "1"
        self.side = torch.cuda.Stream(device=self.dev) if side else None
        # trailing launches (the head's weight-gradient tiles, a layer's slice reduce) parked and appended to the next backward
        # chain launch as extra workgroups on its idle CUs (include/raindrop_hip.h rd_set_defer_trailing).  Also in the two-graph
        # data-parallel form: every part ends with rd_flush_trailing (_body), so the last layer's reduce -- whose results the first
        # gradient bucket's all-reduce needs between the graphs -- is launched on its own at the end of graph A instead of riding
        # in graph B; the head's tiles ride inside A, layer 0's reduce inside B.  RD_TRAILING_RIDE=0: every launch on its own (A/B).
        self.ride = has_backward and self.side is None and os.environ.get("RD_TRAILING_RIDE", "1") != "0"
        # token plan: the step's fast paths only (fused message passing, row-block encoder; the TRAINING head's backward,
        # rd_masked_mean_bwd, does not follow a plan, so a step with a backward needs the fused head for it)
        self._want_plan = (os.environ.get("RD_TOKEN_PLAN", "1") != "0") if token_plan is None else bool(token_plan)
        self.plan = None
        if self._want_plan and (self.head_fused or not has_backward) and self._plan_supported():
            self.plan = torch.zeros(max(int(self.lib.rd_token_plan_bytes(self.sp)) // 4, 64), dtype=torch.int32, device=self.dev)
        # all weight splits of the step in one launch (rd_step_prepare) where the shape takes prepared tiles
        enc_ok, k1_ok = ctypes.c_int32(0), ctypes.c_int32(0)
        _lib.call("rd_step_prepare_covers", self.sp, ctypes.byref(enc_ok), ctypes.byref(k1_ok))
        one = os.environ.get("RD_STEP_PREPARE", "1") != "0"
        self.one_begin = os.environ.get("RD_STEP_BEGIN", "1") != "0"      # A/B: token plan and weight splits as one launch
        self.prep_enc, self.prep_k1 = bool(enc_ok.value) and one, bool(k1_ok.value) and one and sensor.prepared_tiles
        self._prep_w = (ctypes.POINTER(_lib.RdEncoderPtrs) * self.nl)(*[ctypes.pointer(w) for w in self.enc_w])
        self._prep_saved = (ctypes.c_void_p * self.nl)(*[t.data_ptr() for t in self.enc_saved])
        self._prep_bytes = (ctypes.c_size_t * self.nl)(*[t.numel() for t in self.enc_saved])
        self._ptrs = self._param_ptrs()                          # the captured graph / cached structs hold these addresses

    def _param_ptrs(self):
        return tuple(p.data_ptr() for p in self.P.values()) + tuple(g.data_ptr() for g in self.G.values())

    def _plan_supported(self):
        m = self.model
        return plan_supported(m.d_inp, m.d_ob, self.T, self.D, m.nhead, m.nhid, self.lib.rd_get_precision())

    def _alloc(self, crit=None, focal=None):
        """Every buffer of the step, in the arena's order (the offsets are part of the measured step: _Arena).  crit / focal: the
        contents of the criterion buffers (`criterion_values` / `focal_values`), None for a step without that buffer."""
        lib, sp, B, T, D, m, bwd = self.lib, self.sp, self.B, self.T, self.D, self.model, self.has_backward
        self.nl = len(m.transformer_encoder.layers)
        k1_bytes = self.sensor.buffer_bytes(self)
        enc_saved, enc_ws = lib.rd_encoder_layer_saved_bytes(sp), lib.rd_encoder_layer_workspace_bytes(sp)
        if self.infer:                                            # inference sizes; a covered layer does not touch its workspace
            k1_cov, enc_cov = ctypes.c_int32(0), ctypes.c_int32(0)
            _lib.call("rd_infer_covers", sp, ctypes.byref(k1_cov), ctypes.byref(enc_cov))
            self.infer_covers = (bool(k1_cov.value), bool(enc_cov.value))
            enc_saved = lib.rd_encoder_layer_infer_bytes(sp)
            enc_ws = 0 if enc_cov.value else enc_ws
        self._arena = a = _Arena(self.dev, [T * B * D * 4] * (1 + self.nl + (2 if bwd else 0)) + list(k1_bytes)
                                 + [enc_saved] * self.nl + [enc_ws] * self.nl)
        grad = lambda shape: a.zeros(shape) if bwd else None
        self.z = a.zeros((T, B, D))
        self.mask = torch.empty((B, T), dtype=torch.bool, device=self.dev)
        self.k1_saved, self.k1_ws = a.u8(k1_bytes[0]), a.u8(k1_bytes[1])
        self.x = [self.z] + [a.zeros((T, B, D)) for _ in range(self.nl)]
        self.enc_saved = [a.u8(enc_saved) for _ in range(self.nl)]
        # one workspace per layer: a layer's trailing reduce launch (side branch, rd_set_side_stream) reads its partials while the
        # next layer's backward already writes its own
        self.enc_wss = [a.u8(enc_ws) for _ in range(self.nl)]
        self.enc_ws = self.enc_wss[0]
        self.dx = [grad((T, B, D)), grad((T, B, D))]              # ping-pong gradient buffers (_grad_in)
        self.Fe = m.d_inp if m.static else 0
        dh = D + self.Fe
        self.feat, self.dfeat = a.zeros((B, dh)), grad((B, dh))
        self.hid, self.dhid = a.zeros((B, dh)), grad((B, dh))
        self.logits, self.dlogits = a.zeros((B, m.n_classes)), grad((B, m.n_classes))
        self.loss = torch.zeros((), dtype=torch.float32, device=self.dev) if bwd else None
        self.wg_ws = a.u8(max(lib.rd_linear_bwd_weight_workspace_bytes(B, dh, dh),
                              lib.rd_linear_bwd_weight_workspace_bytes(B, m.n_classes, dh),
                              lib.rd_linear_bwd_weight_workspace_bytes(B, max(self.Fe, 1), max(m.d_static, 1)))) if bwd else None
        # classifier head + loss + their backward as two launches (rd_head.hip) when the sizes fit, else operator by operator.
        # Forward-only: the eager surface's head in both layouts (raindrop_amd/evalstep.py has the reason)
        self.head_fused = bwd and bool(lib.rd_head_train_supported(D, self.Fe, m.n_classes))
        self.head_ws = a.u8(lib.rd_head_train_workspace_bytes(B, dh, m.n_classes)) if self.head_fused else None
        # the criterion [eps, w_0 .. w_{C-1}] of a step with class weights / label smoothing (None: the plain mean cross entropy),
        # the focal loss's [gamma, w_0 .. w_{C-1}] of a step built with focal_gamma (then crit is None: one criterion per step)
        filled = lambda vals: None if vals is None else a.zeros((len(vals),)).copy_(torch.tensor(vals, dtype=torch.float32))
        self.crit, self.focal = filled(crit), filled(focal)
        tables = lambda T_: [_lib.RdEncoderPtrs(*[T_["transformer_encoder.layers.%d.%s" % (i, n)].data_ptr() for n in ops.ENC_PARAM_NAMES])
                             for i in range(self.nl)]
        self.enc_w, self.enc_g = tables(self.P), tables(self.G) if bwd else []
        self.sensor.alloc(self)

    # ---- stages: each enqueues on the current stream through self._call, no host sync ------------------------------------------
    def _call(self, name, *a):
        _lib.call(name, *a)

    def _grad_in(self, i):
        """The buffer of the ping-pong pair that holds d loss / d x[i + 1], which layer i's backward READS (and the layer above,
        or the head, wrote): dx[0] for the top layer, alternating downwards; _grad_in(-1) is what the sensor stage reads."""
        return self.dx[(self.nl - 1 - i) % 2]

    def _one_launch_begin(self):
        """the `begin` stage is rd_step_begin (which also advances a registered optimizer step cell: TrainStep.capture_full)"""
        return self.plan is not None and (self.prep_enc or self.prep_k1) and self.one_begin

    def _begin(self):
        """Token plan, seed bump and weight splits: one launch (rd_step_begin) where all three exist, else one each."""
        b, P, sp, st, c = self.batch, self.P, self.sp, ops._stream(), self._call
        W1, W2 = P["ob_propagation.lin_value.weight"], P["ob_propagation_layer2.lin_value.weight"]
        prep = self.prep_enc or self.prep_k1
        prep_args = (self.nl if self.prep_enc else 0, self._prep_w, self._prep_saved, self._prep_bytes,
                     _p(W1) if self.prep_k1 else None, _p(W2) if self.prep_k1 else None, _p(self.k1_saved), self.k1_saved.numel(), st)
        drops = self.p_drop > 0.0 or self.sensor.edge_drop                 # (either sensor stage's coefficient dropout)
        cell = _p(self.seed_cell) if drops else None
        if self._one_launch_begin():
            return c("rd_step_begin", sp, _p(b["lengths"]), _p(self.plan), cell, 1, *prep_args)
        if self.plan is not None:                                          # lengths -> token plan (+ the seed bump: one launch)
            c("rd_token_plan", sp, _p(b["lengths"]), _p(self.plan), cell, 1, st)
        elif drops:
            c("rd_seed_cell_advance", _p(self.seed_cell), 1, st)           # fresh masks per replay
        if prep:
            c("rd_step_prepare", sp, *prep_args)

    def _sensor_fwd(self):
        self.sensor.forward(self, ops._stream())                           # -> self.z, self.mask

    def _sensor_bwd(self):
        self.sensor.backward(self, self._grad_in(-1), ops._stream())

    def _enc_fwd(self):
        for i in range(self.nl):
            if self.infer:
                self._call("rd_encoder_layer_fwd_infer", self.sp, i | (0x10000 if self.prep_enc else 0), _p(self.x[i]), _p(self.mask),
                           ctypes.byref(self.enc_w[i]), _p(self.x[i + 1]), _p(self.enc_saved[i]), self.enc_saved[i].numel(),
                           _p(self.enc_wss[i]), self.enc_wss[i].numel(), ops._stream())
                continue
            self._call("rd_encoder_layer_fwd", self.sp, i | (0x10000 if self.prep_enc else 0), _p(self.x[i]), _p(self.mask),
                       ctypes.byref(self.enc_w[i]), self.p_drop, self.seed, _p(self.x[i + 1]), _p(self.enc_saved[i]),
                       self.enc_saved[i].numel(), _p(self.enc_wss[i]), self.enc_wss[i].numel(), ops._stream())

    def _enc_bwd(self, hi, lo):
        """Backward of encoder layers hi .. lo."""
        for i in range(hi, lo - 1, -1):
            self._call("rd_encoder_layer_bwd", self.sp, i, _p(self.x[i]), _p(self.mask), ctypes.byref(self.enc_w[i]), self.p_drop,
                       self.seed, _p(self.enc_saved[i]), self.enc_saved[i].numel(), _p(self._grad_in(i)), _p(self._grad_in(i - 1)),
                       ctypes.byref(self.enc_g[i]), _p(self.enc_wss[i]), self.enc_wss[i].numel(), ops._stream())

    def _enc_bwd_top(self):                                                # the last layer's backward closes part 'a'
        self._enc_bwd(self.nl - 1, self.nl - 1)

    def _enc_bwd_rest(self):
        self._enc_bwd(self.nl - 2, 0)

    def _fused_head_args(self):
        """The argument list the three fused head kernels share: (inputs and weights, [gradients ..., entry gradient, workspace,
        its size, stream]); rd_head_forward takes the last three of the second."""
        m, b, P, G, Fe = self.model, self.batch, self.P, self.G, self.Fe
        e = lambda T_, n: _p(T_[n]) if Fe else None
        w = lambda T_: (e(T_, "emb.weight"), e(T_, "emb.bias")) + tuple(_p(T_["mlp_static." + n]) for n in ("0.weight", "0.bias", "2.weight", "2.bias"))
        return ((self.sp, self.D, m.d_static if Fe else 0, Fe, m.n_classes, _p(self.x[-1]), _p(self.mask), _p(b["lengths"]),
                 _p(b["static"]) if Fe else None) + w(P),
                (w(G) if G else ()) + (_p(self._grad_in(self.nl - 1)), _p(self.head_ws), self.head_ws.numel(), ops._stream()))

    def _loss_entry(self):
        """(entry-point suffix, device buffer) of the step's loss: `criterion_entry` of its two buffers"""
        return criterion_entry(self.focal, self.crit)

    def _head_train(self):
        """Classifier head + mean cross entropy and their backward, down to the encoder stack's entry gradient."""
        if not self.head_fused:
            return self._head_by_operator()
        common, tail = self._fused_head_args()
        suffix, buf = self._loss_entry()                                    # the plain, criterion or focal instantiation
        self._call("rd_head_train" + suffix, *common, _p(self.batch["y"]), *_spliced(buf), _p(self.loss), _p(self.logits), *tail)

    def set_criterion(self, class_weight=None, label_smoothing=0.0, focal_gamma=None):
        """Change the step's loss to CrossEntropyLoss(weight=class_weight, label_smoothing=label_smoothing) between steps: a copy of
        C + 1 floats into the device buffer the head kernels read when they run, like `lr` -- never a new capture.  None / 0 mean
        what they mean to the constructor (all weights 1 / no smoothing).  Only a step BUILT with a criterion has that buffer and
        the kernels that read it; any other refuses (build a new step).
        A step built with focal_gamma takes `class_weight` and `focal_gamma` the same way (its buffer is [gamma, w_0 ..]); it
        refuses label_smoothing, and a call without focal_gamma; a step not built focal refuses focal_gamma."""
        suffix, buf = self._loss_entry()
        if suffix == "_focal":
            check_focal(label_smoothing, 0.0 if focal_gamma is None else focal_gamma)
            if focal_gamma is None:
                raise _lib.RaindropHipError("set_criterion: this step was built for the focal loss (focal_gamma=...) and its captured "
                                            "head runs the focal kernels; pass focal_gamma=... (0.0 is the weighted cross entropy), "
                                            "or build a new step for another criterion")
            vals = focal_values(class_weight, focal_gamma, self.model.n_classes)
        elif focal_gamma is not None:
            raise _lib.RaindropHipError("set_criterion: this step was not built for the focal loss (focal_gamma=None) and its captured "
                                        "head reads no gamma; build the step with focal_gamma=... to change it between steps")
        elif buf is None:
            raise _lib.RaindropHipError("set_criterion: this step was built for the plain mean cross entropy (class_weight=None, "
                                        "label_smoothing=0) and its captured head reads no criterion buffer; build the step with "
                                        "class_weight=... or label_smoothing=... to change them between steps")
        else:
            vals = criterion_values(class_weight, label_smoothing, self.model.n_classes) or [0.0] + [1.0] * self.model.n_classes
        buf.copy_(torch.tensor(vals, dtype=torch.float32))

    def _head_fwd(self):
        """The head around a loss the caller evaluates (or none): up to self.logits."""
        if not self.head_fused:
            return self._head_forward_by_operator()
        common, tail = self._fused_head_args()
        self._call("rd_head_forward", *common, _p(self.logits), *tail[-3:])

    def _head_bwd(self):
        """From self.dlogits, which the caller fills: the head's parameter gradients and the encoder stack's entry gradient."""
        if not self.head_fused:
            raise _lib.RaindropHipError("part 'mb' needs the fused head (rd_head_backward) and a step with a backward")
        common, tail = self._fused_head_args()
        self._call("rd_head_backward", *common, _p(self.dlogits), *tail)

    def _head_by_operator(self):
        """masked mean -> [agg | emb] -> mlp_static -> cross entropy and their backward, one C-ABI call per operator."""
        m, b, P, G, sp, st = self.model, self.batch, self.P, self.G, self.sp, ops._stream()
        B, D, Fe, C = self.B, self.D, self.Fe, m.n_classes
        dh = D + Fe
        c = self._call
        self._head_forward_by_operator()
        # ---------------- loss: mean cross entropy (code/Raindrop.py:255,322) and its gradient ----------
        suffix, buf = self._loss_entry()
        c("rd_softmax_xent" + suffix, B, C, _p(self.logits), _p(b["y"]), *_spliced(buf), _p(self.loss), _p(self.dlogits), st)
        # ---------------- backward ----------------
        ws, wsn = _p(self.wg_ws), self.wg_ws.numel()
        c("rd_linear_bwd_weight", B, C, dh, _p(self.dlogits), C, _p(self.hid), dh, _p(G["mlp_static.2.weight"]),
          _p(G["mlp_static.2.bias"]), ws, wsn, st)
        c("rd_linear_bwd_input_gated", B, C, dh, _p(self.dlogits), C, _p(P["mlp_static.2.weight"]), _p(self.hid), dh,
          _p(self.dhid), dh, st)                                             # ReLU gate of mlp_static[1] folded in
        c("rd_linear_bwd_weight", B, dh, dh, _p(self.dhid), dh, _p(self.feat), dh, _p(G["mlp_static.0.weight"]),
          _p(G["mlp_static.0.bias"]), ws, wsn, st)
        c("rd_linear_bwd_input", B, dh, dh, _p(self.dhid), dh, _p(P["mlp_static.0.weight"]), _p(self.dfeat), dh, st)
        if Fe:
            demb = self.dfeat[:, D:]
            c("rd_linear_bwd_weight", B, Fe, m.d_static, ctypes.c_void_p(demb.data_ptr()), dh, _p(b["static"]),
              m.d_static, _p(G["emb.weight"]), _p(G["emb.bias"]), ws, wsn, st)
        c("rd_masked_mean_bwd", sp, D, _p(self.dfeat), dh, _p(self.mask), _p(b["lengths"]), _p(self._grad_in(self.nl - 1)), st)

    def _head_forward_by_operator(self):
        """The forward half of `_head_by_operator`, up to the logits: the calls the eager model makes (models_rd.py forward)."""
        m, b, P, sp, st = self.model, self.batch, self.P, self.sp, ops._stream()
        B, D, Fe, C = self.B, self.D, self.Fe, m.n_classes
        dh = D + Fe
        c = self._call
        c("rd_masked_mean_fwd", sp, D, _p(self.x[-1]), _p(self.mask), _p(b["lengths"]), _p(self.feat), dh, st)
        if Fe:
            emb_out = self.feat[:, D:]                                       # right block of [agg | emb]
            c("rd_linear_fwd", B, Fe, m.d_static, _p(b["static"]), m.d_static, _p(P["emb.weight"]), _p(P["emb.bias"]),
              ctypes.c_void_p(emb_out.data_ptr()), dh, 0, st)
        c("rd_linear_fwd", B, dh, dh, _p(self.feat), dh, _p(P["mlp_static.0.weight"]), _p(P["mlp_static.0.bias"]),
          _p(self.hid), dh, 1, st)
        c("rd_linear_fwd", B, C, dh, _p(self.hid), dh, _p(P["mlp_static.2.weight"]), _p(P["mlp_static.2.bias"]),
          _p(self.logits), C, 0, st)

    def _stages(self, part=None):
        for stage in self.PARTS[part]:
            getattr(self, "_" + stage)()

    def _body(self, part=None):
        """The stages of `part` + the join of the side branch: launches forked inside this part (weight-gradient reduces, the
        head's weight gradients: rd_set_side_stream) are complete, in stream order, when the part is."""
        self._stages(part)
        _lib.call("rd_flush_trailing", ops._stream())              # a parked trailing launch nobody picked up (layer 0's reduce)
        _lib.call("rd_side_join", ops._stream())

    def _with_cell(self, fn):
        """Run `fn` with this step's token plan and -- with a backward -- seed cell, side stream and trailing riders registered.
        The registration is read when a kernel is ENQUEUED (the pointer travels as a kernel argument), so it is scoped to the
        enqueue / the capture: a captured graph keeps the cell it was captured with, and nothing else in the process (an eager
        model, another step) ever sees this step's cell -- dropping a step can not leave a dangling pointer behind."""
        regs = [("rd_set_token_plan", _p(self.plan), None)]
        if self.has_backward:
            regs = [("rd_set_seed_cell", _p(self.seed_cell), None), regs[0],
                    ("rd_set_side_stream", ctypes.c_void_p(self.side.cuda_stream) if self.side is not None else None, None),
                    ("rd_set_defer_trailing", 1 if self.ride else 0, 0)]
        for name, on, _ in regs:
            _lib.call(name, on)
        try:
            return fn()
        finally:
            for name, _, off in regs:
                _lib.call(name, off)


class TrainStep(Step):
    # candidates of the autotune in _capture (masks of rd_set_rowgemm_rows32 / rd_set_rowgemm_waves16): the workgroup heights are
    # timed at TUNE_WAVES[0], then the other wave masks at the best height.  tests/test_rowgemm_variants_gpu.py runs every pair.
    TUNE_HEIGHTS = (15, 0, 3, 12)
    TUNE_WAVES = (12, 15)

    def __init__(self, model, flat, batch, p_drop=None, use_graph=True, seed=1234, autotune=True, token_plan=None, split=None,
                 module_mode=False, sensor=None, class_weight=None, label_smoothing=0.0, feed=None, accumulate=1, focal_gamma=None):
        """model: raindrop_amd.models_rd.Raindrop_v2 on a ROCm device; flat: FlatGradAllReduce over the
        live parameters (its buffer receives the gradients); batch: dict(src, static, times, lengths, y)
        of device tensors that are REUSED every step (copy new data into them).
        feed: a raindrop_amd.feed.EpochFeed -- the step fetches its own batch: in every form (eager run(), the captured graph, the
        two-graph form, capture_full) the FIRST thing enqueued, in front of the `begin` stage, is rd_feed_gather, which copies batch
        `cursor` of the feed's epoch plan into `batch`, and the LAST (behind the optimizer in capture_full, at the end of the second
        graph in the two-graph form) is rd_feed_record, which stores this batch's loss and number of correct predictions in the
        feed's history and advances the cursor.  run() / run_full() refuse once `feed.remaining()` is 0.  The warm-up passes of a
        capture run the step for real: the feed's cursor, history and counter are put back afterwards, `batch` holds whatever they
        gathered.  The measurement captures (capture_segments / capture_marked) do not feed.  None: the launches the step always
        enqueued.
        class_weight, label_smoothing: the loss is torch.nn.CrossEntropyLoss(weight=class_weight, label_smoothing=label_smoothing)
        instead of the plain mean cross entropy, in every form of the step (eager run(), the captured graph, capture_full, the
        two-graph data-parallel form); `set_criterion` changes both between replays without a new capture.  Each rank normalises by
        the weights of its OWN shard's labels and the gradient all-reduce averages the ranks -- DistributedDataParallel's result
        with torch's criterion, not the single-process result on the global batch (`Step.__init__`).
        focal_gamma: the focal loss with these class weights in every form of the step (`Step.__init__`, `focal_values`); needs
        label_smoothing == 0; `set_criterion(class_weight=, focal_gamma=)` changes it between replays.  Under accumulate=k each
        micro-batch is normalised by its own weight sum, and each rank by its own shard's, as with class weights.
        token_plan: store and process only the live (sample, step) rows (include/raindrop_hip.h "token plan": the padding mask of
        code/models_rd.py:298-299 applied as a layout; same logits, loss and gradients).  None = environment RD_TOKEN_PLAN
        (default on) where the shape supports it.
        sensor: the sensor-stage object (default: the default branch's; BetaTrainStep passes the use_beta one).
        accumulate: k micro-batches per optimizer step (an int >= 1; 1, the default: the step as it always was, no accumulator).
        With k > 1 the step owns `acc`, an fp32 accumulator the size of flat.flat (zero at construction), and `scale_cell`, one
        float32 holding 1/k, and every form is captured twice: positions 0 .. k-2 of a window end with rd_grad_accumulate
        (acc += g), position k-1 with rd_grad_accumulate_close (g = (acc + g) * scale, acc = 0).  `window_position()` is the
        host's count of micro-batches in the open window; `window_closed` says whether the last call closed one -- that is when
        flat.flat holds the window's gradient and the caller steps the optimizer.
          * the window's gradient is the MEAN of the k micro-batch gradients, each normalised by its own denominator (its batch
            size, or under class weights its own weight sum): what torch users get from `(loss / k).backward()` k times;
          * the dropout seed cell, the feed's cursor and its loss / correct records advance per micro-batch; the optimizer's step
            count, its schedule position and its EMA count per window; `max_grad_norm` sees the norm of the window's mean, and a
            window with a non-finite micro-batch is skipped as a whole (the accumulator is clean afterwards);
          * `p.grad` views hold the window's mean after a closing call and the LAST micro-batch's own gradient otherwise;
          * data parallel: every rank accumulates locally, `run_allreduce()` issues NO collective on positions 0 .. k-2 and the
            closing call's collective averages the ranks' window means (DistributedDataParallel's no_sync);
          * `module_mode=True` refuses k > 1: the loss is the caller's there, and autograd's own accumulation already works."""
        if isinstance(accumulate, bool) or not isinstance(accumulate, int) or accumulate < 1:
            raise ValueError("accumulate must be an integer >= 1, got %r" % (accumulate,))
        if accumulate > 1 and module_mode:
            raise ValueError("TrainStep(module_mode=True) leaves the loss and its backward to the caller, whose autograd accumulates "
                             "by itself: accumulate=%d is refused" % accumulate)
        self.accumulate, self.acc, self.scale_cell, self._pos, self.window_closed = accumulate, None, None, 0, False
        # module_mode (raindrop_amd.graph_module): the loss is the CALLER's -- the step is cut into parts 'mf' (forward up to the
        # logits) and 'mb' (backward from self.dlogits, which the caller fills), batch carries no labels
        self.module_mode = bool(module_mode)
        if feed is not None and self.module_mode:
            raise ValueError("TrainStep(module_mode=True) takes its batch and its loss from the caller: it can not run on a feed")
        # split: capture the step as TWO graphs -- (A) forward + loss + the backward of the head and the last encoder layer, (B) the
        # rest of the backward pass -- so that a data-parallel caller can start the all-reduce of the gradients A has finished
        # (run(between=...)) beside B.  None = on when torch.distributed runs more than one rank (RD_DP_OVERLAP=0 turns it off).
        if split is None:
            import torch.distributed as dist
            split = (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
                     and os.environ.get("RD_DP_OVERLAP", "1") != "0")
        self.split = bool(split) and len(model.transformer_encoder.layers) >= 2
        self.autotune, self.tuned_rows32, self.tuned_waves16 = bool(autotune), None, None
        super().__init__(model, batch, sensor or SensorStage(), flat=flat, labels=not self.module_mode, p_drop=p_drop, seed=seed,
                         token_plan=token_plan, class_weight=class_weight, label_smoothing=label_smoothing, focal_gamma=focal_gamma)
        if self.split:
            self._check_split_order()
        self.feed = feed
        if feed is not None:
            feed.check_step(model, batch)
        self.graph = self.graph_b = self.graph_full = self._full_opt = self._full_hyper = None
        self.graph_close = self.graph_b_close = self.graph_full_micro = None   # accumulate > 1: the closing twins of graph / graph_b,
        self.captures = 0                                                  # the micro twin of graph_full; whole-step graphs captured so far
        if accumulate > 1:                                                 # (not in the arena: accumulate=1 allocates what it always did)
            self.acc = torch.zeros_like(flat.flat)
            self.scale_cell = torch.full((1,), 1.0 / accumulate, dtype=torch.float32, device=self.dev)
        if use_graph:
            with self._feed_kept():
                self._capture()

    # ---- the feed's two launches around the step (nothing without a feed) ---------------------------------------------------------
    def _feed_gather(self):
        if self.feed is not None:
            self.feed.enqueue_gather(self.batch, self._call)

    def _feed_record(self):
        if self.feed is not None:
            self.feed.enqueue_record(self.loss, self.logits, self.batch["y"], self._call)

    @contextlib.contextmanager
    def _feed_kept(self):
        """around a capture: its warm-up passes (and the autotune's timed replays) gather, record and advance the cursor like any
        step -- the feed is as it was afterwards, and so is the accumulator of an open window (accumulate > 1: the passes end with
        the accumulate and close launches)"""
        snap = self.feed.snapshot() if self.feed is not None else None
        acc = self.acc.clone() if self.acc is not None else None
        try:
            yield
        finally:
            if snap is not None:
                self.feed.restore(snap)
            if acc is not None:
                self.acc.copy_(acc)

    # ---- the window's launch behind the body (nothing with accumulate == 1) -------------------------------------------------------
    def _window_tail(self, closing, part=None):
        """What follows part `part` of the body on a window position: behind the whole step (None) or behind 'b' the accumulate
        launch over the whole buffer (positions 0 .. k-2) or the close launch (position k-1) -- over the whole buffer, or in the
        split form over the range each part completes: [early_grad_offset(), n) behind 'a', so that the first bucket's collective
        reads the window's mean, and [0, offset) behind 'b'.  (The offset is a multiple of 64 elements: dp.FlatGradAllReduce.)"""
        if self.acc is None:
            return
        g, n = self.flat.flat, self.flat.flat.numel()
        if not closing:
            if part != "a":
                self._call("rd_grad_accumulate", n, _p(g), _p(self.acc), ops._stream())
            return
        off = self.early_grad_offset() if part is not None else 0
        lo, hi = (off, n) if part == "a" else (0, off) if part == "b" else (0, n)
        if hi > lo:
            self._call("rd_grad_accumulate_close", hi - lo, ctypes.c_void_p(g.data_ptr() + 4 * lo),
                       ctypes.c_void_p(self.acc.data_ptr() + 4 * lo), _p(self.scale_cell), ops._stream())

    def _closing_next(self):
        """the next call closes a window (always, without accumulation)"""
        return self._pos == self.accumulate - 1

    def _advance_window(self, closing):
        self._pos = 0 if closing else self._pos + 1
        self.window_closed = bool(closing)

    def window_position(self):
        """micro-batches taken in the open window, 0 .. accumulate - 1 (host count: no synchronisation)"""
        return self._pos

    def reset_window(self):
        """Drop the open window: the accumulator is zeroed (stream-ordered) and the next call is position 0."""
        if self.acc is not None:
            self.acc.zero_()
        self._pos, self.window_closed = 0, False

    def _capture(self):
        """Capture the step as one hipGraph (two in the split form).  With `autotune`, the step is captured once per setting of the
        library's tuning knobs (32-row vs 64-row workgroups of the encoder's row-block products, rd_set_rowgemm_rows32, then 8 vs
        16 waves for the plain ones: which is faster depends on the device, 8 % either way was measured on two boxes of one pool)
        and the fastest kept.  Under torch.distributed every rank times every variant and the per-variant times are SUMMED over
        the ranks before the choice, so all ranks run the same kernels -- and the same ones a single process would pick on such
        boxes.  The choice is in `tuned_rows32` / `tuned_waves16` (bench.py: config.tuned).
        Results: the knobs change which rows share a workgroup, never a row's arithmetic; on the fused row-local chains
        (rd_encfuse.hip: the P19 / P12 widths) no cross-row sum depends on them, so every variant gives the same gradient bits.
        On the unfused LayerNorm-epilogue products (other widths) the dgamma / dbeta partial grouping follows the workgroup
        height: there the bits depend on the choice, which is why it is recorded (pin it with RD_RG_ROWS32 / RD_RG_WAVES16).
        Held by tests/test_rowgemm_variants_gpu.py: every TUNE_HEIGHTS x TUNE_WAVES pair (and the four corner masks) against the
        default masks on the row-block path -- output, input gradient and all weight / bias gradients bit-identical, the four
        LayerNorm affine gradients within 2e-5 of their max-norm."""
        import torch.distributed as dist
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        if not self.autotune or os.environ.get("RD_RG_ROWS32") is not None or os.environ.get("RD_RG_WAVES16") is not None:
            return self._capture_one()

        def agree(ts):
            """per-variant times summed over the ranks (identical on every rank afterwards)"""
            if not multi:
                return ts
            dev = self.dev if dist.get_backend() == "nccl" else torch.device("cpu")
            t = torch.tensor(ts, dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            return [float(v) for v in t.cpu()]

        def timed(r32, w16):
            _lib.call("rd_set_rowgemm_rows32", r32)
            _lib.call("rd_set_rowgemm_waves16", w16)
            graphs = self._capture_one()                             # (timed: the first two, a non-closing position)

            def replay():
                graphs[0].replay()
                if graphs[1] is not None:
                    graphs[1].replay()
            for _ in range(3):
                replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(30):
                replay()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0, graphs)
        # workgroup height first (all / none / plain products only / LayerNorm-fused ones only) at the default wave counts,
        # then the wave count of the plain products at the best height
        heights = self.TUNE_HEIGHTS
        runs = [timed(r32, self.TUNE_WAVES[0]) for r32 in heights]
        ts = agree([r[0] for r in runs])
        bi = min(range(len(heights)), key=lambda i: (ts[i], i))
        best_r32, best_w16, best_graphs, best_t = heights[bi], self.TUNE_WAVES[0], runs[bi][1], ts[bi]
        for w16 in self.TUNE_WAVES[1:]:
            alt = timed(best_r32, w16)
            alt_t = agree([alt[0]])[0]
            if alt_t < best_t:
                best_w16, best_graphs, best_t = w16, alt[1], alt_t
        self.graph, self.graph_b, self.graph_close, self.graph_b_close = best_graphs
        self.tuned_rows32, self.tuned_waves16 = best_r32, best_w16
        _lib.call("rd_set_rowgemm_rows32", best_r32)                 # eager calls of this process follow the same choice
        _lib.call("rd_set_rowgemm_waves16", best_w16)


    def _parts(self):
        """the parts a micro-batch is enqueued in: the two halves of the split form -- 'a' ends where the gradients from
        early_grad_offset() on are final --, else the step as one piece"""
        return ("a", "b") if self.split else (None,)

    def _enqueue(self, closing=True, parts=None, after_part=None, opt=None):
        """THE order of a micro-batch, for every form of the step: feed gather | per part: body, the window's launch, `after_part(part)`
        (what a caller puts behind a part: `between`, a collective) | feed record.  `parts`: `_parts()`, or (None,): the step as one
        piece whatever `split` says (the warm-up passes, capture_full's micro graph), or ONE of 'a', 'b': that half alone, for a
        graph of its own -- the gather goes in front of 'a', the record behind 'b'.  `opt` (capture_full's closing pass): the
        optimizer's update behind the last part, in front of the record; its step cell is registered from the gather to the first
        body where the `begin` stage advances it (`_one_launch_begin`), else the update advances it itself."""
        parts = self._parts() if parts is None else parts
        if parts[0] != "b":
            self._feed_gather()
            if opt is not None and self._one_launch_begin():
                opt.register_cell(True)
        for k, part in enumerate(parts):
            self._body(part)
            if opt is not None and k == 0:
                opt.register_cell(False)
            self._window_tail(closing, part)
            if after_part is not None:
                after_part(part)
        if parts[-1] != "a":
            if opt is not None:
                opt.step_captured(advance=not self._one_launch_begin())
            self._feed_record()

    def _warm(self, after_part=None):
        """What every capture of the step warms up with, whatever it captures: the step as ONE piece (the split forms too), under
        accumulation a non-closing position and then a closing one."""
        if self.acc is not None:
            self._enqueue(False, parts=(None,))
        self._enqueue(True, parts=(None,), after_part=after_part)

    def _capture_one(self):
        """`graph` (+ `graph_b`, split form): the step.  With accumulate > 1 these are the graphs of a window's positions 0 .. k-2
        and `graph_close` (+ `graph_b_close`) those of position k-1: the same body captured twice, out of one pool.  Returns the four."""
        bodies = [lambda c=closing, p=part: self._enqueue(c, parts=(p,))
                  for closing in ((False, True) if self.acc is not None else (True,)) for part in self._parts()]
        graphs = self._with_cell(lambda: capture_graphs(bodies, warm=self._warm))
        n, pair = len(self._parts()), lambda gs: (gs + [None, None])[:2]
        self.graph, self.graph_b, self.graph_close, self.graph_b_close = pair(graphs[:n]) + pair(graphs[n:])
        return self.graph, self.graph_b, self.graph_close, self.graph_b_close

    def capture_segments(self, parts=("begin", "k1f", "mid", "k1b")):
        """The same step as consecutive hipGraphs, one per part (measurement only: bench.py brackets the 'k1f' / 'k1b' replays with
        HIP events, so the message-passing launches are timed with the cache state, clocks and neighbours they have in the step).
        Replaying the graphs in order is one step."""
        return self._with_cell(lambda: capture_graphs([lambda pt=pt: self._body(pt) for pt in parts]))

    def capture_marked(self, parts=("begin", "k1f", "enc", "head", "encb", "k1b")):
        """The step as ONE hipGraph with an external timing event recorded in front of every part and behind the last
        (torch.cuda.Event(enable_timing=True, external=True): event-record NODES of the graph): per-part device times of the real
        step, without the ~10 us a graph boundary costs per segment.  Returns (graph, events); raises where the runtime cannot
        capture external event records (callers fall back to capture_segments)."""
        events = [torch.cuda.Event(enable_timing=True, external=True) for _ in range(len(parts) + 1)]

        def parts_only():
            for pt in parts:
                self._body(pt)

        def marked():
            for k, pt in enumerate(parts):
                events[k].record()
                self._body(pt)
            events[len(parts)].record()
        return self._with_cell(lambda: capture_graphs([marked], warm=parts_only))[0], events

    # ------------------------------------------------------------------------------------------
    # ------------------------------------------------------------------------------------------
    def _early_names(self):
        """Parameters whose gradients the first all-reduce bucket of the split form carries: the last encoder layer's and the
        classifier head's (mlp_static).  (The static embedding's gradient is complete by then too, but sits in front of the
        offset in forward order and travels with the rest: early completion is harmless, late completion is not.)"""
        pre = "transformer_encoder.layers.%d." % (self.nl - 1)
        return [n for n in self.flat.names if n.startswith(pre) or n.startswith("mlp_static.")]

    def _check_split_order(self):
        """Ordering contract of the split (overlapped all-reduce) form: in the flat buffer every gradient the first graph completes
        must sit at or behind early_grad_offset(), and nothing the SECOND graph writes (R_u, ob_propagation*, earlier encoder
        layers, emb) may sit there -- the collective started between the graphs would read it while graph B is still writing.
        raindrop_amd.synth.live_parameter_names (forward order) satisfies it; model.named_parameters() order does NOT
        (R_u and ob_propagation* are registered behind transformer_encoder, code/models_rd.py:241-247)."""
        names = list(self.flat.names)
        first = "transformer_encoder.layers.%d.self_attn.in_proj_weight" % (self.nl - 1)
        if first not in names:
            raise _lib.RaindropHipError("TrainStep(split=True): %s is not in the flat gradient buffer" % first)
        i0 = names.index(first)
        early = set(self._early_names())
        bad_tail = [n for n in names[i0:] if n not in early]
        bad_head = [n for n in names[:i0] if n in early]
        if bad_tail or bad_head:
            raise _lib.RaindropHipError(
                "TrainStep(split=True): the flat gradient buffer must hold the parameters in FORWARD order "
                "(raindrop_amd.synth.live_parameter_names): behind %s only the last encoder layer and mlp_static may follow; "
                "found %s behind it and %s in front of it.  Pass split=False (or RD_DP_OVERLAP=0) for another order."
                % (first, bad_tail[:4], bad_head[:4]))

    def early_grad_offset(self):
        """Offset in the flat gradient buffer from which every gradient is final when `between` runs (split form): the last encoder
        layer's parameters and, behind them in forward order, the classifier head's."""
        return self.flat.tail_start("transformer_encoder.layers.%d.self_attn.in_proj_weight" % (self.nl - 1))

    def run(self, between=None):
        """One forward + loss + backward; gradients land in flat.flat (p.grad views point there).  `between` (split form only) is
        called after the first graph has been enqueued and before the second: gradients at flat offsets >= early_grad_offset() are
        complete in stream order at that point.
        accumulate > 1: one MICRO-batch.  On positions 0 .. k-2 of a window flat.flat holds this micro-batch's own gradient
        afterwards (and the accumulator has taken it in); on position k-1 it holds the window's mean -- at `between`, already from
        early_grad_offset() on -- and `window_closed` is True: step the optimizer."""
        if self._param_ptrs() != self._ptrs:
            raise _lib.RaindropHipError("TrainStep: a parameter or gradient buffer moved since construction (model.to(), "
                                        "flatten_parameters() or a re-assignment): build a new TrainStep")
        if self.feed is not None:
            self.feed._take("TrainStep.run")
        closing = self._closing_next()
        if self.graph is not None:
            first, second = (self.graph_close, self.graph_b_close) if closing and self.acc is not None else (self.graph, self.graph_b)
            first.replay()
            if second is not None:
                if between is not None:
                    between()
                second.replay()
        else:
            after = None if between is None else (lambda part: between() if part == "a" else None)
            with torch.no_grad():
                self._with_cell(lambda: self._enqueue(closing, after_part=after))
        self._advance_window(closing)
        for p, v in zip(self.flat.params, self.flat.views):
            p.grad = v
        return self.loss

    def run_allreduce(self):
        """run() + the gradient all-reduce of `flat` (no-op for one process).  Split form: the collective of the gradients the first
        graph completes (last encoder layer + head: ~0.8 of 2.0 MB at P19) is started between the two graphs and runs beside the
        rest of the backward pass; the remainder follows the second graph.  Returns the loss tensor.
        accumulate > 1: only the call that closes a window reduces (the window's mean; in the split form with the same overlap);
        on the other positions no collective is issued at all.  `window_closed` tells the caller which it was."""
        if not self._closing_next():
            return self.run()
        collective = self._collectives()
        loss = self.run(between=lambda: collective("a"))
        collective("b" if self.split else None)
        return loss

    def _collectives(self):
        """The gradient all-reduce of a closing pass as an `after_part` of `_enqueue`: behind the whole step flat.allreduce(); in the
        split form [early_grad_offset(), n) started behind 'a', beside the rest of the backward pass, and [0, offset) behind 'b',
        then both waited for, in that order."""
        flat, started = self.flat, []

        def after(part):
            if part is None:
                return flat.allreduce()
            off = self.early_grad_offset()
            started.append(flat.allreduce_range_async(off, flat.flat.numel()) if part == "a" else flat.allreduce_range_async(0, off))
            if part == "b":
                while started:
                    flat.allreduce_wait(started.pop(0))
        return after


    # ------------------------------------------------------------------------------------------
    def capture_full(self, opt):
        """The WHOLE step as ONE hipGraph (round 5; opt-in): forward + loss + backward, the gradient all-reduce(s) and the optimizer.
        At N > 1 the first bucket's collective (last encoder layer + head) is started between the two halves of the backward and
        joined behind the second one's -- the collectives' own stream forks from and joins the captured stream (RCCL supports
        stream capture; tested on a one-rank group: tests/test_dp_gpu.py) --, then `opt.step_captured()` (FlatAdam: device step
        cell + rd_adam_step_dev).  The host side of a step is then ONE replay (run_full).  Raises whatever the capture raises;
        the caller falls back to run_allreduce() + opt.step().
        accumulate > 1: TWO graphs out of one pool -- `graph_full_micro` for positions 0 .. k-2 of a window (feed gather, body,
        rd_grad_accumulate, feed record: the optimizer's step cell is not registered, no collective, no update) and `graph_full`
        for position k-1, which is the graph above with rd_grad_accumulate_close in front of the collective(s).  The accumulator
        and the window position are kept across the capture."""
        flat = self.flat
        opt.sync_cells(full=True)                                          # the device step state and the cells of whatever the optimizer has on
        # the optimizer's device step state is advanced by the step's FIRST launch (rd_step_begin, next to the seed bump) where
        # the step has that launch -- registered for the capture only --, else by a one-thread launch in front of the update
        # (`_enqueue`).  The warm-up runs a real flat.allreduce(): outside the capture, RCCL's lazy inits too.
        # positions 0 .. k-2 (accumulate > 1): the step as one piece -- the optimizer's cell is not registered (its step state
        # stays), no collective, no update
        bodies = [lambda: self._enqueue(False, parts=(None,))] if self.acc is not None else []
        bodies.append(lambda: self._enqueue(True, after_part=self._collectives(), opt=opt))

        def cap():
            try:
                return capture_graphs(bodies, warm=lambda: self._warm(lambda part: flat.allreduce()))
            finally:
                opt.register_cell(False)
        with self._feed_kept():
            self.graph_full_micro, self.graph_full = ([None] + self._with_cell(cap))[-2:]
        opt.sync_step_cell()                                               # the warm-up did not step the optimizer; neither did the capture
        self._full_opt = opt
        self._full_hyper = opt.hyper()                                     # betas, eps are launch arguments: baked into the graph (lr, weight decay: device cell)
        self.captures += 1
        return self.graph_full

    def run_full(self, close_window=False):
        """One replay of capture_full's graph = one training step including the optimizer; returns the loss tensor.
        accumulate > 1: one MICRO-batch -- a replay of the micro graph on positions 0 .. k-2 of a window, of the closing graph (the
        collectives, the update; `opt.t`, the schedule and the EMA count move) on position k-1; the optimizer's cells are synchronised
        and its host count advanced on closing replays only.  close_window=True closes the window with THIS micro-batch wherever
        it stands (an epoch's last, shorter window): 1 / (position + 1) goes into the scale cell (a stream-ordered 4-byte write),
        the closing graph is replayed and 1/k is put back."""
        if self.graph_full is None:
            raise _lib.RaindropHipError("TrainStep.run_full: call capture_full(opt) first")
        if self._param_ptrs() != self._ptrs:
            raise _lib.RaindropHipError("TrainStep: a parameter or gradient buffer moved since construction: build a new TrainStep")
        self._full_opt.check_can_step("TrainStep.run_full")               # FlatAdam.swap_ema / ema_weights(): the parameters ARE the average now
        if self.feed is not None:
            self.feed._take("TrainStep.run_full")
        if self._full_opt.hyper() != self._full_hyper:                     # betas / eps changed: launch constants of the captured
            cell = self.seed_cell.clone()                                  # Adam -- capture again
            self.capture_full(self._full_opt)                              # (the warm-up passes advance the dropout stream: put it back)
            self.seed_cell.copy_(cell)
        closing = bool(close_window) or self._closing_next()
        if not closing:                                                    # (accumulate > 1) nothing of the optimizer's moves
            self.graph_full_micro.replay()
        else:
            self._full_opt.sync_cells()                                    # lr / weight decay (ReduceLROnPlateau, code/Raindrop.py:257-259; warm-up /
                                                                           # cosine schedules), threshold, decay: 8-byte copies, no new capture; and
                                                                           # the step state, when host-side steps were taken since
            short = not self._closing_next()                               # a window cut short: the mean over the micro-batches it has
            if short:
                self.scale_cell.fill_(1.0 / (self._pos + 1))
            self.graph_full.replay()
            if short:
                self.scale_cell.fill_(1.0 / self.accumulate)
            self._full_opt.note_replay()
        self._advance_window(closing)
        for p, v in zip(self.flat.params, self.flat.views):
            p.grad = v
        return self.loss

    def close(self):
        """Kept for callers of the round-1 API: the seed cell is no longer registered outside run() / capture."""
        self.graph = self.graph_b = self.graph_full = self.graph_close = self.graph_b_close = self.graph_full_micro = None


class AutogradStep:
    """Any `Raindrop_v2` -- the paper's branch (`use_beta=True` / `compute_distance=True`), which `TrainStep` refuses, included -- as ONE
    hipGraph per training step: `model.forward -> CrossEntropyLoss -> loss.backward() -> Adam` exactly as code/Raindrop.py:319-324
    runs them, through the module's own autograd surface (one C-ABI call per operator), captured once with static input buffers and
    replayed.  Same kernels, same results as the eager loop (the capture only removes the host from the replay path); dropout masks
    change per replay through a device seed cell the graph bumps itself, as in `TrainStep`.

    This is the composed form of the use_beta path (obs embed -> lin_value / increase_dim -> LDS graph operator -> per-sample edge
    softmax -> layer 2 -> tokens: ~7 launches for the sensor stage, DESIGN.md (e')), not a fused kernel; `bench.py --use-beta`
    times it.  The optimizer is torch's own Adam in its capturable fused form over the model's parameters (the reference's
    `torch.optim.Adam(model.parameters(), lr)`, code/Raindrop.py:256), inside the graph; `lr` is a device tensor there, so a
    scheduler can change it without a new capture.

    `distance_weight` (lambda): the captured step minimises the paper's objective `CE + lambda * distance` instead, the
    structure-distance regulariser code/models_rd.py:345-346 returns (differentiable on `use_beta=True, compute_distance=True`:
    rd_structure_distance_bwd -> rd_graph_beta_bwd_alpha).  Any other model would add lambda * 0 and is refused.  0: CE alone,
    the same capture as without the argument."""

    def __init__(self, model, batch, lr=1e-4, optimizer=True, seed=1234, distance_weight=0.0, class_weight=None, label_smoothing=0.0,
                 focal_gamma=None):
        """class_weight / label_smoothing (`criterion_values`): the captured loss is torch.nn.functional.cross_entropy(logits, y,
        weight=class_weight, label_smoothing=label_smoothing) (`_criterion`).  focal_gamma (`focal_values`; label_smoothing must be
        0): the focal loss with these class weights, written in torch operations."""
        crit = criterion_values(class_weight, label_smoothing, model.n_classes)
        check_focal(label_smoothing, focal_gamma)
        focal = None if focal_gamma is None else focal_values(class_weight, focal_gamma, model.n_classes)
        self.model, self.batch = model, batch
        self.dev = batch["src"].device
        self._crit = None if crit is None else (crit[0], torch.tensor(crit[1:], dtype=torch.float32, device=self.dev))
        self._focal = None if focal is None else (focal[0], torch.tensor(focal[1:], dtype=torch.float32, device=self.dev))
        self.distance_weight = float(distance_weight)
        if self.distance_weight != 0.0 and not (getattr(model, "use_beta", False) and getattr(model, "compute_distance", False)):
            raise _lib.RaindropHipError("AutogradStep(distance_weight=%g): the structure distance is the constant 0 unless the model "
                                        "has use_beta=True and compute_distance=True (code/models_rd.py:317,345-346)"
                                        % self.distance_weight)
        validate_batch(model, batch)
        self.seed_cell = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.opt = None
        if optimizer:
            self.opt = torch.optim.Adam(self.params, lr=torch.tensor(float(lr), device=self.dev), capturable=True, fused=True)
        self.loss = torch.zeros((), dtype=torch.float32, device=self.dev)
        self.logits = None
        self.distance = None
        model.graph_step = False                                  # the operator surface is what gets captured
        self._capture()

    def _criterion(self, logits, y):
        """The step's cross entropy.  Without smoothing it is torch's own call (with `weight` when given).  With smoothing AND
        weights torch's fused call cannot be captured: its weighted mean gathers the weights through `masked_select`, whose
        output size is read back on the host ("operation not permitted when stream is capturing").  The same value -- mean
        reduction, no ignore_index -- written out in operations of static shape:
            (1 - eps) sum_b w[y_b] (-logp[b,y_b]) / W + (eps / C) sum_b sum_c w_c (-logp[b,c]) / W,   W = sum_b w[y_b]."""
        focal = getattr(self, "_focal", None)
        if focal is not None:
            # sum_b w[y_b] q_b^gamma (-logp[b,y_b]) / W with q_b the summed probability of the other classes (rd_softmax_xent_focal)
            gamma, w = focal
            if gamma == 0.0:
                return torch.nn.functional.cross_entropy(logits, y, weight=w)
            logp = torch.log_softmax(logits, 1)
            hot = torch.nn.functional.one_hot(y, logits.shape[1]).to(logp.dtype)
            q = (logp.exp() * (1.0 - hot)).sum(1)
            wy = w[y]
            return -(wy * q.pow(gamma) * (logp * hot).sum(1)).sum() / wy.sum()
        if self._crit is None:
            return torch.nn.functional.cross_entropy(logits, y)
        eps, w = self._crit
        if eps == 0.0:
            return torch.nn.functional.cross_entropy(logits, y, weight=w)
        logp = torch.log_softmax(logits, 1)
        wy = w[y]
        W = wy.sum()
        nll = -(wy * logp.gather(1, y.unsqueeze(1)).squeeze(1)).sum() / W
        smooth = -(logp * w).sum() / W
        return (1.0 - eps) * nll + (eps / logits.shape[1]) * smooth

    def _one(self):
        b = self.batch
        logits, distance, _ = self.model(b["src"], b["static"], b["times"], b["lengths"])
        loss = self._criterion(logits, b["y"])
        if self.distance_weight != 0.0:
            loss = loss + self.distance_weight * distance
        loss.backward()
        if self.opt is not None:
            self.opt.step()
        return logits, distance, loss

    def _capture(self):
        def one_pass():
            for p in self.params:
                p.grad = None
            self._one()
        _lib.call("rd_set_seed_cell", _p(self.seed_cell))
        try:
            warm_up(one_pass, passes=3, no_grad=False)             # lazy initialisations, the optimizer's state tensors
            for p in self.params:
                p.grad = None                                      # the captured backward ALLOCATES the gradients (static addresses)
            # (not capture_graphs: autograd stays on, and the gradients are reset between the warm-up and the capture)
            self.graph = torch.cuda.CUDAGraph()
            with _graph_capture(self.graph):
                _lib.call("rd_seed_cell_advance", _p(self.seed_cell), 1, ops._stream())
                logits, distance, loss = self._one()
                self.loss_static, self.logits, self.distance = loss.detach(), logits.detach(), distance.detach()
        finally:
            _lib.call("rd_set_seed_cell", None)

    def run(self):
        self.graph.replay()
        return self.loss_static

    def close(self):
        self.graph = None
