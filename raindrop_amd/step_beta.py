"""Static training step for the paper's branch, `Raindrop_v2(use_beta=True)`: `TrainStep`'s machinery -- one hipGraph per step,
gradients written straight into the flat buffer, `FlatAdam` / `capture_full`, the token plan, the two-graph data-parallel form --
around the use_beta sensor stage.

`TrainStep` with its default sensor stage refuses this branch; the only other captured form of the paper's model is `AutogradStep`,
the module's autograd surface replayed (encoder and head operator by operator in the padded layout, torch's Adam, ~25 ATen
fillers).  Nothing behind the sensor stage is specific to the default branch: it needs `z` and `mask` in the step's layout.
What differs is `BetaSensorStage`, the sensor-stage object a step asks (raindrop_amd/step.py): validation, buffer sizes, the extra
buffers, the forward (`rd_beta_stage_fwd`) and the backward (`rd_beta_stage_bwd`, raindrop_amd/csrc/rd_beta_stage.hip), and no K1
tiles from rd_step_prepare.  `BetaTrainStep` is `TrainStep` constructed with it -- `rd_encoder_layer_fwd/bwd` on the fused
chains, `rd_head_train`, the trailing riders, the autotune of the row-block variants, `run` / `run_allreduce` / `capture_full` /
`run_full` / `close` are TrainStep's --, and `EvalStep` (raindrop_amd/evalstep.py) uses the same object without a backward.

    flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names_beta(cfg)])
    step = BetaTrainStep(model, flat, batch, distance_weight=lam)        # lam only with compute_distance=True
    step.capture_full(FlatAdam(flat.flatten_parameters(), lr))
    loss = step.run_full()                                               # step.loss: the CE term; step.distance: the distance
"""
import ctypes

import torch

from . import _lib, ops
from .models_rd import edge_dropout_of
from .step import SensorStage, TrainStep, _p

BETA_EXTRA = ("ob_propagation.increase_dim.weight", "ob_propagation.increase_dim.bias", "ob_propagation.map_weights")


class BetaSensorStage(SensorStage):
    """The sensor stage of `Raindrop_v2(use_beta=True)`.  distance_weight != 0 (fixed at construction: it selects the backward that
    gets captured) pushes lambda * d distance through the graph operator; lambda itself lives in the device cell `lam_cell`.
    Coefficient dropout: `pe1`, the model's `ob_propagation.dropout` read when the step is built (training-mode model and a step
    with a backward; an evaluation step never drops), selects rd_beta_stage_fwd_dropout / _bwd_dropout
    (`ob_propagation_layer2.dropout > 0` is refused, raindrop_amd.models_rd.edge_dropout_of); the masks follow the step's seed and seed cell like the model's own dropout (fresh per replay, the rank offset in
    the data-parallel form)."""
    prepared_tiles = False        # rd_step_prepare's K1 weight tiles belong to the default branch's fused stage

    def __init__(self, distance_weight=0.0):
        self.distance_weight, self.with_distance = float(distance_weight), float(distance_weight) != 0.0
        self.pe1 = 0.0

    @property
    def edge_drop(self):
        """the step draws coefficient-dropout masks: its seed cell must advance per replay even with the model's dropout at 0"""
        return self.pe1 > 0.0

    def check(self, model):
        if not getattr(model, "use_beta", False):
            raise _lib.RaindropHipError("BetaTrainStep implements Raindrop_v2(use_beta=True) only; the default branch runs on TrainStep")
        if model.d_ob != 4 or model.d_pe != 16 or model.d_inp > 1024:
            raise _lib.RaindropHipError("BetaTrainStep: the use_beta stage needs d_ob = 4, d_pe = 16 and at most 1024 sensors "
                                        "(got %d, %d, %d)" % (model.d_ob, model.d_pe, model.d_inp))

    def buffer_bytes(self, step):
        """step.k1_saved / step.k1_ws are the use_beta stage's buffers (the forward uses the workspace, too)"""
        E = ctypes.c_int32(int(step.graph_info["edge_index"].shape[1]))
        if step.infer:                                            # beta, p_t, kept; X .. y2 live in the workspace's backward scratch
            return int(step.lib.rd_beta_stage_infer_bytes(step.sp, E)), int(step.lib.rd_beta_stage_workspace_bytes(step.sp, E))
        return int(step.lib.rd_beta_stage_saved_bytes(step.sp, E)), int(step.lib.rd_beta_stage_workspace_bytes(step.sp, E))

    def alloc(self, step):
        g, dev = step.graph_info, step.dev
        if step.has_backward:
            self.pe1 = edge_dropout_of(step.model)
            if not 0.0 <= self.pe1 < 1.0:
                raise _lib.RaindropHipError("BetaTrainStep: ob_propagation.dropout must be in [0, 1), got %r" % (self.pe1,))
        self.ei = g["edge_index"].contiguous()                    # [2,E] int64, rows E apart
        self.ew = g["edge_weights"].contiguous()
        self.E = int(self.ei.shape[1])
        ops._validate_edges(self.ei, step.model.d_inp, "BetaTrainStep")
        self.Kk = int(step.lib.rd_graph_beta_kept(self.E))
        self.ei2 = torch.zeros((step.B, 2, self.Kk), dtype=torch.int64, device=dev)
        self.alpha = torch.zeros((step.B, self.Kk), dtype=torch.float32, device=dev)
        self.distance = torch.zeros((), dtype=torch.float32, device=dev)
        self.lam_cell = torch.full((1,), self.distance_weight, dtype=torch.float32, device=dev)

    def forward(self, s, st):
        b, P = s.batch, s.P
        l1, l2 = "ob_propagation.", "ob_propagation_layer2."
        drop = (self.pe1,) if self.edge_drop else ()
        if s.infer:
            return s._call("rd_beta_stage_fwd_infer", s.sp, _p(b["src"]), _p(b["times"]), _p(b["lengths"]), _p(s.ts), _p(P["R_u"]),
                           _p(P[l1 + "lin_value.weight"]), _p(P[l1 + "lin_value.bias"]), _p(P[l1 + "increase_dim.weight"]),
                           _p(P[l1 + "increase_dim.bias"]), _p(P[l1 + "map_weights"]), _p(P[l2 + "lin_value.weight"]),
                           _p(P[l2 + "lin_value.bias"]), _p(self.ei), self.E, _p(self.ew), self.E, _p(s.z), _p(s.mask), _p(self.ei2),
                           _p(self.alpha), _p(self.distance) if s.model.compute_distance else None, _p(s.k1_saved),
                           s.k1_saved.numel(), _p(s.k1_ws), s.k1_ws.numel(), st)
        s._call("rd_beta_stage_fwd_dropout" if self.edge_drop else "rd_beta_stage_fwd", s.sp, _p(b["src"]), _p(b["times"]),
                _p(b["lengths"]), _p(s.ts), _p(P["R_u"]),
                _p(P[l1 + "lin_value.weight"]), _p(P[l1 + "lin_value.bias"]), _p(P[l1 + "increase_dim.weight"]),
                _p(P[l1 + "increase_dim.bias"]), _p(P[l1 + "map_weights"]), _p(P[l2 + "lin_value.weight"]), _p(P[l2 + "lin_value.bias"]),
                _p(self.ei), self.E, _p(self.ew), self.E, s.p_drop, *drop, s.seed, _p(s.z), _p(s.mask), _p(self.ei2),
                _p(self.alpha), _p(self.distance) if s.model.compute_distance else None, _p(s.k1_saved), s.k1_saved.numel(),
                _p(s.k1_ws), s.k1_ws.numel(), st)

    def backward(self, s, cur, st):
        b, P, G = s.batch, s.P, s.G
        l1, l2 = "ob_propagation.", "ob_propagation_layer2."
        drop = (self.pe1, s.seed) if self.edge_drop else ()
        s._call("rd_beta_stage_bwd_dropout" if self.edge_drop else "rd_beta_stage_bwd", s.sp, _p(b["src"]), _p(P["R_u"]),
                _p(P[l1 + "lin_value.weight"]),
                _p(P[l1 + "increase_dim.weight"]), _p(P[l1 + "map_weights"]), _p(P[l2 + "lin_value.weight"]), _p(self.ei), self.E,
                _p(self.ew), self.E, s.p_drop, *drop, _p(self.ei2), _p(self.alpha), _p(s.k1_saved), s.k1_saved.numel(),
                _p(cur), s.D, _p(self.lam_cell) if self.with_distance else None, _p(G["R_u"]),
                _p(G[l1 + "lin_value.weight"]), _p(G[l1 + "lin_value.bias"]), _p(G[l1 + "increase_dim.weight"]),
                _p(G[l1 + "increase_dim.bias"]), _p(G[l1 + "map_weights"]), _p(G[l2 + "lin_value.weight"]),
                _p(G[l2 + "lin_value.bias"]), _p(s.k1_ws), s.k1_ws.numel(), st)


class BetaTrainStep(TrainStep):
    def __init__(self, model, flat, batch, p_drop=None, use_graph=True, seed=1234, autotune=True, token_plan=None, split=None,
                 distance_weight=0.0, class_weight=None, label_smoothing=0.0, feed=None, accumulate=1, focal_gamma=None):
        """As `TrainStep`, for `Raindrop_v2(use_beta=True)` (with or without `compute_distance`) only.  `flat` must cover the
        branch's live parameters (raindrop_amd.synth.live_parameter_names_beta).
        accumulate: as in `TrainStep` (k micro-batches per optimizer step; the window's gradient is the mean of the k gradients of
        CE + lambda * distance; `self.loss` / `self.distance` are the last micro-batch's).
        feed: as in `TrainStep` (raindrop_amd.feed.EpochFeed: the step gathers its own batch and records loss and accuracy).
        class_weight, label_smoothing: as in `TrainStep` -- the CE term becomes torch's weighted, smoothed criterion (per rank: its
        own shard's weight sum), the objective CE_crit + lambda * distance; the distance term is untouched.
        focal_gamma: as in `TrainStep` -- the CE term becomes the focal loss with these class weights; the distance term is untouched.
        distance_weight (lambda, `compute_distance=True` only): the step minimises CE + lambda * distance, the paper's objective
        (code/models_rd.py:345-346, code/Raindrop.py:319).  `self.loss` stays the CE term, `self.distance` holds the distance, both
        device tensors.  lambda lives in a device cell (`set_distance_weight`): changing it needs no new capture.  0: CE alone --
        the backward is then exactly the CE-only one (no zero-valued cotangent is pushed through the graph operator)."""
        stage = BetaSensorStage(distance_weight)
        stage.check(model)
        self.distance_weight = stage.distance_weight
        if stage.with_distance and not getattr(model, "compute_distance", False):
            raise _lib.RaindropHipError("BetaTrainStep(distance_weight=%g): the structure distance is the constant 0 unless the model "
                                        "has use_beta=True and compute_distance=True (code/models_rd.py:317,345-346)"
                                        % self.distance_weight)
        missing = [n for n in BETA_EXTRA if n not in flat.names]
        if missing:
            raise _lib.RaindropHipError("BetaTrainStep: the flat gradient buffer lacks %s -- build it over "
                                        "raindrop_amd.synth.live_parameter_names_beta(cfg)" % ", ".join(missing))
        super().__init__(model, flat, batch, p_drop=p_drop, use_graph=use_graph, seed=seed, autotune=autotune, token_plan=token_plan,
                         split=split, sensor=stage, class_weight=class_weight, label_smoothing=label_smoothing, feed=feed,
                         accumulate=accumulate, focal_gamma=focal_gamma)
        self.alpha, self.ei2, self.distance, self.beta_saved, self.beta_ws = stage.alpha, stage.ei2, stage.distance, self.k1_saved, self.k1_ws

    def set_distance_weight(self, lam):
        """Change lambda of CE + lambda * distance between steps (a 4-byte copy into the device cell the captured backward reads)."""
        if not self.sensor.with_distance:
            raise _lib.RaindropHipError("BetaTrainStep.set_distance_weight: the step was built for the CE loss alone (distance_weight=0); "
                                        "build it with a non-zero weight to train CE + lambda * distance")
        self.distance_weight = float(lam)
        self.sensor.lam_cell.fill_(self.distance_weight)
