"""Forward-only captured step: what `TrainStep` / `BetaTrainStep` are to a training step, for evaluation.

The reference validates after every epoch (`code/Raindrop.py:345-370`: `evaluate_standard` -> the whole split through
`model.forward`).  On this project's eager surface that is one C-ABI call per operator in the PADDED layout with fresh allocations
per chunk.  `EvalStep` is the forward half of the captured training step -- the same enqueue code (`TrainStep._body_impl(part="mf")`:
token plan + weight tiles, sensor stage, encoder layers, classifier head up to the logits; `BetaTrainStep._k1_fwd` for the paper's
branch) -- with every buffer allocated once and ONE hipGraph replay per chunk:

    step = EvalStep(model, batch)            # batch: dict(src, times, lengths[, static]) of reused device tensors, no labels
    batch["src"].copy_(...); ...             # new data goes into the same buffers
    logits = step.run()                      # [B, n_classes]; step.distance with use_beta + compute_distance

* nothing of the backward exists: no flat gradient buffer, no `dx` / `dfeat` / weight-gradient workspaces, no gradient pointers;
  parameters, `p.grad`, optimizer state and dropout seed cells are neither written nor registered;
* dropout is off whatever `model.training` says, and the model's mode is left as found;
* the graph reads the parameters by ADDRESS and rebuilds the per-step weight tiles in its first launch, as the training step does:
  an optimizer step or `load_state_dict` between replays is seen by the next replay.  Moved parameters (`model.to(...)`) raise;
* token plan (live `(sample, step)` rows only) where `plan_supported` allows it, padded layout otherwise;
* the classifier head runs operator by operator in BOTH layouts (`rd_masked_mean_fwd`, which follows the plan, and the
  `rd_linear_fwd` calls of the eager model), not as the fused `rd_head_forward`: that kernel is fp32 FMA in every arithmetic mode
  while the eager head follows the mode (split-bf16 products by default), a difference of 2e-6 .. 5e-6 on the logits -- more than
  the whole token plan costs.  With the operator head the step enqueues the eager surface's head: in the padded layout the logits
  are bit-identical to `model.eval(); model.forward(...)`, on the plan they differ by the plan's summation orders at most
  (tests/test_eval_step_gpu.py has the measured figures).  Three small launches more per chunk than the fused head;
* the forward kernels still write their save-for-backward buffers (DESIGN.md "EvalStep" has the share); skipping those writes is
  the follow-up.
"""
import os

import torch

from . import _lib
from .step import TrainStep, _graph_capture, _p
from .step_beta import BetaTrainStep


class _ForwardOnly:
    """Mixed in FRONT of TrainStep / BetaTrainStep: their shape set-up, buffers (`forward_only`: no backward ones), plan / weight-tile
    set-up, `_k1_fwd` and `_body_impl("mf")` are used as they are; construction, capture and `run` are the forward's own."""
    forward_only = True
    plan_needs_fused_head = False                                 # rd_masked_mean_fwd follows the plan

    def _init_forward(self, model, batch, token_plan, use_graph):
        self.model, self.flat, self.batch = model, None, batch
        self.module_mode, self.split = True, False                # part 'mf': the forward ends at the logits
        self.autotune, self.tuned_rows32, self.tuned_waves16 = False, None, None   # the process's row-block knobs stay as they are
        self.dev = batch["src"].device
        self.lib = _lib.load()
        self.p_drop, self.seed = 0.0, 0                           # evaluation: dropout off, whatever model.training says
        self.distance_weight, self._with_distance = 0.0, False
        self._validate(model, batch, labels=False)
        want = (os.environ.get("RD_TOKEN_PLAN", "1") != "0") if token_plan is None else bool(token_plan)
        self._setup_shapes({})
        self._want_plan = want and self._plan_supported()
        self.head_fused = False                                   # the eager surface's head in both layouts (module docstring)
        self.seed_cell, self.side, self.ride = None, None, False
        self._setup_plan_and_prepare()
        self._ptrs = self._param_ptrs()
        self.graph = self.graph_b = None
        self.captures = 0
        if use_graph:
            self._with_cell(self._capture_forward)

    def _head_module(self, cur, st, backward):
        if backward:
            raise _lib.RaindropHipError("EvalStep has no backward")
        return self._head_forward_by_operator(st)

    def _with_cell(self, fn):
        """The token plan is registered for the enqueue only; the seed cell, side stream and trailing riders of the training step
        (dropout and backward-side) are not touched."""
        _lib.call("rd_set_token_plan", _p(self.plan))
        try:
            return fn()
        finally:
            _lib.call("rd_set_token_plan", None)

    def _forward(self):
        self._body_impl("mf")

    def _capture_forward(self):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):                                    # warm-up: lazy inits happen here
                self._forward()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), _graph_capture(self.graph):
            self._forward()
        self.captures += 1

    def run(self):
        if self._param_ptrs() != self._ptrs:
            raise _lib.RaindropHipError("EvalStep: a parameter moved since construction (model.to() or a re-assignment): build a new EvalStep")
        if self.graph is not None:
            self.graph.replay()
        else:
            def eager():
                with torch.no_grad():
                    self._forward()
            self._with_cell(eager)
        return self.logits


class _DefaultEval(_ForwardOnly, TrainStep):
    def __init__(self, model, batch, token_plan, use_graph):
        self._init_forward(model, batch, token_plan, use_graph)

    def _k1_buffer_bytes(self):
        saved, _ = super()._k1_buffer_bytes()                     # rd_msgpass_workspace_bytes is the backward's
        return saved, 0


class _BetaEval(_ForwardOnly, BetaTrainStep):
    def __init__(self, model, batch, token_plan, use_graph):
        self._init_forward(model, batch, token_plan, use_graph)

    def _setup_plan_and_prepare(self):
        super()._setup_plan_and_prepare()
        self.prep_k1 = False                                      # rd_step_prepare's K1 weight tiles belong to the default branch


class EvalStep:
    """EvalStep(model, batch, token_plan=None, use_graph=True): the forward of `Raindrop_v2` -- default branch or `use_beta=True`,
    with or without `compute_distance` -- as one captured graph over reused input buffers (module docstring).
    `run()` -> `logits` [B, n_classes] (the step's own buffer: copy what must outlive the next run); `distance`: the structure
    distance of the last run (use_beta + compute_distance), else None.  `plan`: the token plan tensor or None (padded layout);
    `head_fused`; `captures`: hipGraph captures made so far."""

    def __init__(self, model, batch, token_plan=None, use_graph=True):
        src = batch.get("src") if isinstance(batch, dict) else None
        if src is None or not torch.is_tensor(src) or not src.is_cuda:
            raise _lib.RaindropHipError("EvalStep needs a batch of ROCm device tensors (src, times, lengths[, static]); there is no "
                                        "CPU fallback")
        cls = _BetaEval if getattr(model, "use_beta", False) else _DefaultEval
        self._impl = cls(model, batch, token_plan, use_graph)
        self.model, self.batch = model, batch

    logits = property(lambda self: self._impl.logits)
    plan = property(lambda self: self._impl.plan)
    head_fused = property(lambda self: self._impl.head_fused)
    graph = property(lambda self: self._impl.graph)
    captures = property(lambda self: self._impl.captures)
    B = property(lambda self: self._impl.B)

    @property
    def distance(self):
        m = self.model
        return self._impl.distance if (getattr(m, "use_beta", False) and getattr(m, "compute_distance", False)) else None

    def run(self):
        return self._impl.run()

    def buffer_bytes(self):
        """Bytes of device memory the step holds (activations, saved / workspace buffers, plan), for DESIGN.md's table."""
        i = self._impl
        arena = getattr(i, "_arena", None)
        return int(arena.numel()) if arena is not None else None

    def close(self):
        self._impl.graph = None
