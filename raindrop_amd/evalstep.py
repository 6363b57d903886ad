"""Forward-only captured step: what `TrainStep` / `BetaTrainStep` are to a training step, for evaluation.

The reference validates after every epoch (`code/Raindrop.py:345-370`: `evaluate_standard` -> the whole split through
`model.forward`).  On this project's eager surface that is one C-ABI call per operator in the PADDED layout with fresh allocations
per chunk.  `EvalStep` is the forward half of the captured training step -- `raindrop_amd.step.Step` built with
`has_backward=False` and the sensor-stage object of the model's branch, enqueueing part 'mf' of `Step.PARTS`: token plan + weight
tiles, sensor stage, encoder layers, classifier head up to the logits -- with every buffer allocated once and ONE hipGraph replay
per chunk:

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
* the forward is the INFERENCE forward of every stage (`rd_sensor_stage_fwd_infer` / `rd_beta_stage_fwd_infer`,
  `rd_encoder_layer_fwd_infer`): save-free instantiations of the fused kernels where `rd_infer_covers` reports them (the P19 class),
  the saving kernels elsewhere.  Nothing that only a backward reads is written, and `saved` shrinks to the forward's weight tiles
  plus what one forward launch hands to the next (DESIGN.md "EvalStep" has the sizes and the timing).  The logits -- and `distance`
  -- are bit-identical to the saving form, the training forward with its save-for-backward buffers, which `save_free=False` builds
  (tests/test_infer_forward_gpu.py).  `feed.evaluate_captured` / `feed.validate` ask for the inference form; the CONSTRUCTOR's
  default is the saving form, because tests/golden/step_launches.json records the launches of a default-constructed `EvalStep`
  and that fixture is never regenerated: pass `save_free=True`.
"""
import torch

from . import _lib
from .step import SensorStage, Step, capture_graphs
from .step_beta import BetaSensorStage


class EvalStep(Step):
    """EvalStep(model, batch, token_plan=None, use_graph=True, save_free=False): the forward of `Raindrop_v2` -- default branch or `use_beta=True`,
    with or without `compute_distance` -- as one captured graph over reused input buffers (module docstring).
    `run()` -> `logits` [B, n_classes] (the step's own buffer: copy what must outlive the next run); `distance`: the structure
    distance of the last run (use_beta + compute_distance), else None.  `plan`: the token plan tensor or None (padded layout);
    `head_fused`; `captures`: hipGraph captures made so far.  save_free=True: the inference forward on buffers of the inference
    sizes (module docstring; what `feed.validate` builds); False: the training forward and its save-for-backward buffers.  Same
    logits bit for bit."""

    def __init__(self, model, batch, token_plan=None, use_graph=True, save_free=False):
        src = batch.get("src") if isinstance(batch, dict) else None
        if src is None or not torch.is_tensor(src) or not src.is_cuda:
            raise _lib.RaindropHipError("EvalStep needs a batch of ROCm device tensors (src, times, lengths[, static]); there is no "
                                        "CPU fallback")
        sensor = BetaSensorStage() if getattr(model, "use_beta", False) else SensorStage()
        super().__init__(model, batch, sensor, has_backward=False, labels=False, token_plan=token_plan, save_free=save_free)
        self.graph, self.captures = None, 0
        if use_graph:
            self._with_cell(self._capture)

    def _capture(self):
        self.graph, = capture_graphs([lambda: self._stages("mf")])
        self.captures += 1

    @property
    def distance(self):
        m = self.model
        return self.sensor.distance if (getattr(m, "use_beta", False) and getattr(m, "compute_distance", False)) else None

    def run(self):
        if self._param_ptrs() != self._ptrs:
            raise _lib.RaindropHipError("EvalStep: a parameter moved since construction (model.to() or a re-assignment): build a new EvalStep")
        if self.graph is not None:
            self.graph.replay()
        else:
            def eager():
                with torch.no_grad():
                    self._stages("mf")
            self._with_cell(eager)
        return self.logits

    def buffer_bytes(self):
        """Bytes of device memory the step holds (activations, saved / workspace buffers, plan), for DESIGN.md's table."""
        return int(self._arena.buf.numel()) if self._arena.buf is not None else None

    def close(self):
        self.graph = None
