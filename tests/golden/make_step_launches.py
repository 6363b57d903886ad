"""Launch traces of the captured steps: which C-ABI entry points `TrainStep`, `BetaTrainStep` and `EvalStep` enqueue, with which
arguments and on which buffers, form by form -> tests/golden/step_launches.json.

Every enqueue of raindrop_amd/step*.py, evalstep.py, ops.py and optim.py goes through the module attribute `raindrop_amd._lib.call`;
this generator replaces it with a recorder (which still makes the call) and drives the PUBLIC surface only: constructors, `run`,
`capture_segments`, `capture_marked`, `capture_full`.  Per call the trace holds the entry point's name and, per argument,

    an int / float          by value
    a pointer               0 for NULL, "stream" for the current stream's handle, else the ordinal of the address's first
                            appearance in the form's trace (independent of addresses; pins the buffer wiring, the dx ping-pong
                            included)
    byref / ctypes arrays   the token "ref"

A replay is a captured graph, so identical enqueues are identical graphs: a restructuring of the host layer that leaves this file
unchanged has left the steps unchanged.  The fixture is generated ONCE, by the code the restructuring starts from, and never from
restructured code; tests/test_step_launches_gpu.py re-records with the functions below and compares form by form.

    python tests/golden/make_step_launches.py [out.json]          (needs the GPU)
"""
import contextlib
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from raindrop_amd import _lib, dp, synth  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "step_launches.json")
DEV = "cuda"
_CARG = type(ctypes.byref(ctypes.c_int32(0)))


class Recorder:
    def __init__(self):
        self.trace, self.ordinal = [], {}

    def pointer(self, a):
        v = a.value if isinstance(a, ctypes.c_void_p) else a
        v = int(v or 0)
        if v == 0:
            return 0
        if v == int(torch.cuda.current_stream().cuda_stream):
            return "stream"
        return self.ordinal.setdefault(v, len(self.ordinal) + 1)

    def __call__(self, name, *args):
        types = _lib.SIGNATURES[name][1]
        row = [name]
        for a, t in zip(args, types):
            if isinstance(a, (ctypes.Array, _CARG, ctypes.Structure)):
                row.append("ref")
            elif t is ctypes.c_void_p:
                row.append(self.pointer(a))
            elif isinstance(a, ctypes._SimpleCData):
                row.append(a.value)
            elif isinstance(a, (bool, int, float)):
                row.append(a)
            else:
                row.append("ref")
        self.trace.append(row)
        return self.real(name, *args)

    def mark(self, what):
        self.trace.append(["#" + what])


@contextlib.contextmanager
def recording():
    rec = Recorder()
    rec.real = _lib.call
    _lib.call = rec
    try:
        yield rec
    finally:
        _lib.call = rec.real


@contextlib.contextmanager
def environ(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def configs():
    p19, tiny = synth.make_config("P19"), synth.make_config("TINY")
    return {"p19": (p19, 8),                                         # on the token plan, fused head, two encoder layers
            "p19_l1": (dict(p19, nlayers=1), 8),                     # one layer: `split` is forced off
            "tiny": (tiny, 4),                                       # a width outside plan_supported: padded layout
            "tiny_nostatic": (dict(tiny, static=False, d_static=0), 4)}


def make(cfg, B, **kw):
    """(model in training mode with dropout on, device batch) from fixed seeds"""
    from raindrop_amd.models_rd import Raindrop_v2
    if not cfg["static"]:
        kw["static"] = False
    m = Raindrop_v2(cfg["d_inp"], cfg["d_model"], cfg["nhead"], cfg["nhid"], cfg["nlayers"], cfg["dropout"], cfg["max_len"],
                    cfg["d_static"], cfg["MAX"], 0.5, cfg["aggreg"], cfg["n_classes"], synth.make_structure(cfg, "sparse"),
                    sensor_wise_mask=False, **kw)
    synth.fill_params_(m, seed=7)
    m = m.to(DEV).train()
    batch = {k: (None if v is None else v.to(DEV)) for k, v in synth.make_batch(cfg, B, seed=41).items()}
    return m, batch


def flat_of(m, cfg, beta=False):
    named = dict(m.named_parameters())
    names = synth.live_parameter_names_beta(cfg) if beta else synth.live_parameter_names(cfg)
    return dp.FlatGradAllReduce([(n, named[n]) for n in names], n_buckets=2)


def _train(rec, cfg, B, run=True, coef_dropout=None, **kw):
    from raindrop_amd.step import TrainStep
    m, b = make(cfg, B)
    if coef_dropout is not None:                                     # the attributes upstream users set
        m.ob_propagation.dropout, m.ob_propagation_layer2.dropout = coef_dropout
    if kw.get("module_mode"):
        b = {k: v for k, v in b.items() if k != "y"}
    ts = TrainStep(m, flat_of(m, cfg), b, use_graph=False, autotune=False, **kw)
    rec.mark("split=%d plan=%d head_fused=%d" % (ts.split, ts.plan is not None, ts.head_fused))
    if run:
        ts.run(between=lambda: rec.mark("between"))
    return ts


def form_run(rec, cfg, B):
    _train(rec, cfg, B, split=False)


def form_run_split(rec, cfg, B):
    _train(rec, cfg, B, split=True)


def form_run_padded(rec, cfg, B):
    _train(rec, cfg, B, split=False, token_plan=False)


def form_run_no_dropout(rec, cfg, B):
    _train(rec, cfg, B, split=False, p_drop=0.0)


def form_run_head_by_operator(rec, cfg, B):
    with environ(RD_HEAD_FUSED="0"):
        _train(rec, cfg, B, split=False)


def form_segments(rec, cfg, B):
    ts = _train(rec, cfg, B, run=False, split=False)
    ts.capture_segments(("begin", "k1f", "mid", "k1b"))
    ts.close()


def form_segments_module(rec, cfg, B):
    ts = _train(rec, cfg, B, run=False, split=False, module_mode=True)
    if ts.head_fused:                                                # raindrop_amd.graph_module captures these two parts, fused head only
        ts.capture_segments(("mf", "mb"))
    ts.close()


def form_marked(rec, cfg, B):
    ts = _train(rec, cfg, B, run=False, split=False)
    n = len(rec.trace)
    try:
        ts.capture_marked(("begin", "k1f", "enc", "head", "encb", "k1b"))
    except Exception:                                                # the runtime refuses external event records in a capture
        del rec.trace[n:]
        rec.mark("unsupported")
    ts.close()


def form_full(rec, cfg, B):
    from raindrop_amd.optim import FlatAdam
    from raindrop_amd.step import TrainStep
    m, b = make(cfg, B)
    flat = flat_of(m, cfg)
    opt = FlatAdam(flat.flatten_parameters(), lr=1e-3)
    ts = TrainStep(m, flat, b, use_graph=False, autotune=False, split=False)
    ts.capture_full(opt)
    rec.mark("captured")
    ts.run_full()
    ts.close()


def _beta(rec, cfg, B, lam, coef_dropout=None):
    from raindrop_amd.step_beta import BetaTrainStep
    m, b = make(cfg, B, use_beta=True, compute_distance=True)
    if coef_dropout is not None:
        m.ob_propagation.dropout = coef_dropout
    ts = BetaTrainStep(m, flat_of(m, cfg, beta=True), b, use_graph=False, autotune=False, split=False, distance_weight=lam)
    rec.mark("plan=%d head_fused=%d" % (ts.plan is not None, ts.head_fused))
    ts.run()


def form_beta(rec, cfg, B):
    _beta(rec, cfg, B, 0.0)


def form_beta_distance(rec, cfg, B):
    _beta(rec, cfg, B, 0.25)


def _eval(rec, cfg, B, token_plan, **kw):
    from raindrop_amd.evalstep import EvalStep
    m, b = make(cfg, B, **kw)
    es = EvalStep(m, {k: v for k, v in b.items() if k != "y"}, token_plan=token_plan, use_graph=False)
    rec.mark("plan=%d head_fused=%d distance=%d" % (es.plan is not None, es.head_fused, es.distance is not None))
    es.run()
    es.close()


def form_eval(rec, cfg, B):
    _eval(rec, cfg, B, None)


def form_eval_padded(rec, cfg, B):
    _eval(rec, cfg, B, False)


def form_eval_beta(rec, cfg, B):
    _eval(rec, cfg, B, None, use_beta=True, compute_distance=True)


def form_eval_beta_padded(rec, cfg, B):
    _eval(rec, cfg, B, False, use_beta=True)


def _weights(cfg):
    """class weights with one class at 0 (the criterion's denominator leaves its samples out)"""
    return [0.0] + [1.0 + 0.5 * c for c in range(1, cfg["n_classes"])]


def form_run_crit(rec, cfg, B):
    _train(rec, cfg, B, split=False, class_weight=_weights(cfg), label_smoothing=0.1)


def form_run_focal(rec, cfg, B):
    _train(rec, cfg, B, split=False, class_weight=_weights(cfg), focal_gamma=2.0)


def form_run_crit_head_by_operator(rec, cfg, B):
    with environ(RD_HEAD_FUSED="0"):
        form_run_crit(rec, cfg, B)


def form_run_focal_head_by_operator(rec, cfg, B):
    with environ(RD_HEAD_FUSED="0"):
        form_run_focal(rec, cfg, B)


def _runs(rec, ts, n):
    """n more micro-batches of an accumulating step, a mark in front of each"""
    for k in range(n):
        rec.mark("position=%d" % ts.window_position())
        ts.run(between=lambda: rec.mark("between"))


def form_run_accum(rec, cfg, B):
    _runs(rec, _train(rec, cfg, B, split=False, accumulate=3), 2)          # two micro positions and the close


def form_run_accum_split(rec, cfg, B):
    _runs(rec, _train(rec, cfg, B, split=True, accumulate=2), 1)


def _graph(rec, cfg, B, **kw):
    """construction with use_graph=True (warm-up + capture), then one replay"""
    from raindrop_amd.step import TrainStep
    m, b = make(cfg, B)
    ts = TrainStep(m, flat_of(m, cfg), b, use_graph=True, autotune=False, **kw)
    rec.mark("captured split=%d" % ts.split)
    ts.run(between=lambda: rec.mark("between"))
    ts.close()


def form_graph(rec, cfg, B):
    _graph(rec, cfg, B, split=False)


def form_graph_split(rec, cfg, B):
    _graph(rec, cfg, B, split=True)


def form_graph_accum(rec, cfg, B):
    _graph(rec, cfg, B, split=False, accumulate=2)


def form_graph_accum_split(rec, cfg, B):
    _graph(rec, cfg, B, split=True, accumulate=2)


def _full(rec, cfg, B, replays, **kw):
    from raindrop_amd.optim import FlatAdam
    from raindrop_amd.step import TrainStep
    m, b = make(cfg, B)
    flat = flat_of(m, cfg)
    opt = FlatAdam(flat.flatten_parameters(), lr=1e-3)
    ts = TrainStep(m, flat, b, use_graph=False, autotune=False, **kw)
    ts.capture_full(opt)
    rec.mark("captured split=%d" % ts.split)
    for _ in range(replays):
        ts.run_full()
    ts.close()


def form_full_split(rec, cfg, B):
    _full(rec, cfg, B, 1, split=True)


def form_full_accum(rec, cfg, B):
    _full(rec, cfg, B, 2, split=False, accumulate=2)


def form_full_accum_split(rec, cfg, B):
    _full(rec, cfg, B, 2, split=True, accumulate=2)


def _feed(cfg, B):
    """an epoch feed over the smallest dataset that gives two batches, its plan loaded"""
    import numpy as np
    from raindrop_amd import feed
    data = synth.make_batch(cfg, 2 * B, seed=43)
    ds = feed.DeviceDataset(data["src"], data["times"], data["static"], data["y"], device=DEV)
    fd = feed.EpochFeed(ds, B, capacity=2)
    fd.load_epoch([np.arange(B), np.arange(B, 2 * B)])
    return fd


def form_run_feed(rec, cfg, B):
    _train(rec, cfg, B, split=False, feed=_feed(cfg, B))


def form_full_feed(rec, cfg, B):
    _full(rec, cfg, B, 1, split=False, feed=_feed(cfg, B))


def form_run_coef_dropout(rec, cfg, B):
    _train(rec, cfg, B, split=False, coef_dropout=(0.25, 0.125))


def form_beta_coef_dropout(rec, cfg, B):
    _beta(rec, cfg, B, 0.0, coef_dropout=0.25)


FORMS = {"run": form_run, "run_split": form_run_split, "run_padded": form_run_padded, "run_no_dropout": form_run_no_dropout,
         "run_head_by_operator": form_run_head_by_operator, "segments": form_segments, "segments_module": form_segments_module,
         "marked": form_marked, "full": form_full, "beta": form_beta, "beta_distance": form_beta_distance, "eval": form_eval,
         "eval_padded": form_eval_padded, "eval_beta": form_eval_beta, "eval_beta_padded": form_eval_beta_padded,
         # the forms the features since the restructuring into stages added (recorded from the last commit that restated the
         # step's order per form)
         "run_crit": form_run_crit, "run_focal": form_run_focal, "run_crit_head_by_operator": form_run_crit_head_by_operator,
         "run_focal_head_by_operator": form_run_focal_head_by_operator, "run_accum": form_run_accum,
         "run_accum_split": form_run_accum_split, "graph": form_graph, "graph_split": form_graph_split,
         "graph_accum": form_graph_accum, "graph_accum_split": form_graph_accum_split, "full_split": form_full_split,
         "full_accum": form_full_accum, "full_accum_split": form_full_accum_split, "run_feed": form_run_feed,
         "full_feed": form_full_feed, "run_coef_dropout": form_run_coef_dropout, "beta_coef_dropout": form_beta_coef_dropout}
# the captures on the two P19 configurations only (what bench.py and graph_module capture); every enqueued form on every width
CAPTURES = ("segments", "segments_module", "marked", "full", "graph", "graph_split", "graph_accum", "graph_accum_split", "full_split",
            "full_accum", "full_accum_split", "full_feed")


def cases():
    return [(c, f) for c in configs() for f in FORMS if f not in CAPTURES or c.startswith("p19")]


def record(cfg_name, form):
    """The trace of one form on one configuration, in default precision; JSON-ready."""
    cfg, B = configs()[cfg_name]
    _lib.call("rd_set_precision", 1)
    with recording() as rec:
        FORMS[form](rec, cfg, B)
    torch.cuda.synchronize()
    return json.loads(json.dumps(rec.trace))


if __name__ == "__main__":
    out = {}
    for c, f in cases():
        out["%s/%s" % (c, f)] = record(c, f)
        print("%s/%s: %d calls" % (c, f, len(out["%s/%s" % (c, f)])), flush=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as fh:
        fh.write("{\n" + ",\n".join('"%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in out.items()) + "\n}\n")
