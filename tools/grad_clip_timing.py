"""Cost of FlatAdam's gradient clipping / non-finite guard in the whole-step graph: TrainStep.capture_full at P19, B = 256 (the
model, batch, structure and optimizer of bench.py), once with FlatAdam(lr=1e-4) -- the feature off: the launches of a tree without
it -- and once with FlatAdam(lr=1e-4, max_grad_norm=M), M = half the first step's gradient norm (on: rd_grad_sumsq +
rd_adam_step_clip_dev instead of rd_adam_step_dev).  Both steps live in ONE process and are timed in alternating blocks of
`--block` replays (wall clock around a synchronize), so that clocks and neighbours are shared.  Writes one JSON object.

    python tools/grad_clip_timing.py [--batch 256] [--block 100] [--rounds 6] [--warmup 30] [--out profiles/grad_clip_timing.json]
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def build(batch, dev, max_grad_norm):
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
    kw = {} if max_grad_norm is None else {"max_grad_norm": max_grad_norm}
    opt = FlatAdam(flat.flatten_parameters(), lr=1e-4, **kw)
    ts = TrainStep(model, flat, b)
    return ts, flat, opt


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256); ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=6); ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_clip_timing.json"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    ts_off, flat_off, opt_off = build(a.batch, dev, None)
    ts_off.run()
    torch.cuda.synchronize()
    norm0 = float(flat_off.flat.double().norm())
    ts_on, _, opt_on = build(a.batch, dev, 0.5 * norm0)
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
    res = {"workload": "TrainStep.capture_full(FlatAdam), P19 all-ones structure, B=%d, dropout %.1f, one hipGraph replay per step; off: "
                       "FlatAdam(lr=1e-4), on: FlatAdam(lr=1e-4, max_grad_norm=half the first norm)" % (a.batch, ts_off.p_drop),
           "block_steps": a.block, "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "ms_per_step_blocks": blocks, "ms_per_step_mean": {k: round(v, 5) for k, v in mean.items()},
           "off_block_spread_ms": round(max(blocks["off"]) - min(blocks["off"]), 5),
           "on_minus_off_ms": round(mean["on"] - mean["off"], 5), "first_grad_norm": norm0, "on_stats": opt_on.grad_stats(),
           "steps_taken": {"off": opt_off.t, "on": opt_on.t, "on_device": opt_on.device_steps()}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res), flush=True)
    ts_off.close(); ts_on.close()


if __name__ == "__main__":
    main()
