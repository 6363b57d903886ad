"""Cost of class weights / label smoothing in the whole-step graph: TrainStep.capture_full at P19, B = 256 (the model, batch,
structure and optimizer of bench.py), once with the plain mean cross entropy -- the launches of a tree without the feature -- and
once with TrainStep(class_weight=[1, 6], label_smoothing=0.1) (on: the criterion instantiation of the head kernel, rd_head_train_crit).
Both steps live in ONE process and are timed in alternating blocks of `--block` replays (wall clock around a synchronize), so that
clocks and neighbours are shared.  Writes one JSON object (`--bench-ab FILE`: merged under the key "bench_ab", the off-path A/B of
bench.py against the parent commit recorded beside it).

    python tools/ce_criterion_timing.py [--batch 256] [--block 100] [--rounds 6] [--warmup 30] [--out profiles/ce_criterion_timing.json]
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def build(batch, dev, **crit):
    from raindrop_amd import dp, synth
    from raindrop_amd.models_rd import Raindrop_v2
    from raindrop_amd.optim import FlatAdam
    from raindrop_amd.step import TrainStep
    cfg = synth.make_config("P19")
    gs = synth.make_structure(cfg, "ones")
    torch.manual_seed(1)
    model = Raindrop_v2(cfg["d_inp"], cfg["d_model"], cfg["nhead"], cfg["nhid"], cfg["nlayers"], cfg["dropout"], cfg["max_len"],
                        cfg["d_static"], cfg["MAX"], 0.5, cfg["aggreg"], cfg["n_classes"], gs, sensor_wise_mask=False).to(dev).train()
    model.graph_step = False
    b = {k: (None if v is None else v.to(dev)) for k, v in synth.make_batch(cfg, batch, seed=100).items()}
    named = dict(model.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)], n_buckets=2)
    opt = FlatAdam(flat.flatten_parameters(), lr=1e-4)
    ts = TrainStep(model, flat, b, **crit)
    return ts, opt


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256); ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=6); ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--bench-ab", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ce_criterion_timing.json"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    ts_off, opt_off = build(a.batch, dev)
    ts_on, opt_on = build(a.batch, dev, class_weight=[1.0, 6.0], label_smoothing=0.1)
    assert ts_off.crit is None and ts_on.crit is not None and ts_on.head_fused
    steps = {"off": ts_off, "on": ts_on}
    ts_off.capture_full(opt_off)
    ts_on.capture_full(opt_on)
    for ts in steps.values():
        for _ in range(a.warmup):
            ts.run_full()
    torch.cuda.synchronize()
    blocks = {"off": [], "on": []}
    for _ in range(a.rounds):
        for name, ts in steps.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.block):
                loss = ts.run_full()
            torch.cuda.synchronize(); t1 = time.perf_counter()
            assert bool(torch.isfinite(loss))
            blocks[name].append(round((t1 - t0) * 1e3 / a.block, 5))
    mean = {k: sum(v) / len(v) for k, v in blocks.items()}
    res = {"workload": "TrainStep.capture_full(FlatAdam(lr=1e-4)), P19 all-ones structure, B=%d, dropout %.1f, one hipGraph replay per "
                       "step; off: plain mean cross entropy, on: class_weight=[1, 6], label_smoothing=0.1" % (a.batch, ts_off.p_drop),
           "block_steps": a.block, "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "ms_per_step_blocks": blocks, "ms_per_step_mean": {k: round(v, 5) for k, v in mean.items()},
           "off_block_spread_ms": round(max(blocks["off"]) - min(blocks["off"]), 5),
           "on_minus_off_ms": round(mean["on"] - mean["off"], 5), "steps_taken": {"off": opt_off.t, "on": opt_on.t}}
    if a.bench_ab:
        with open(a.bench_ab) as fh:
            res["bench_ab"] = json.load(fh)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res), flush=True)
    ts_off.close(); ts_on.close()


if __name__ == "__main__":
    main()
