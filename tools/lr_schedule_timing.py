"""Cost of a per-step learning-rate schedule, on the device and from the host, in one process: P19, B = 256, a dataset of 3880
samples, the whole step as one hipGraph (`capture_full`) on the epoch feed in all three legs (after tools/feed_graph_timing.py) --

  a  no schedule: `FlatAdam(lr)`, `run_full()` per batch;
  b  the device schedule: `FlatAdam(lr, schedule=LRSchedule.warmup_cosine(...))`, `run_full()` per batch -- the thread that advances
     the step state forms the rate, the host does nothing;
  c  the same rates assigned from the host in front of every replay: `opt.lr = lr * f[k]; run_full()` -- what a caller without the
     feature must do (`sync_cell_hyper`: a tensor construction and an 8-byte host-to-device copy per step).

Wall time per step (host clock around a block that ends in a device synchronise), blocks alternating a b c a b c ... after a warm-up
block of every leg, median / min / max over the blocks; b - a and c - b from the medians, to be read against the legs' own spread.
The three legs run the same plans' worth of steps (`EpochPlanner`, strategy 2, planned in front of the clock).  With `--parent DIR` (a
built checkout of the parent commit) `bench.py` -- the path without a schedule -- is then run alternately in this tree and in DIR,
`--bench-reps` times each: THE MARGIN is the parent's own spread over its processes (min .. max), not a figure fixed here.

    python tools/lr_schedule_timing.py [--blocks 7] [--epochs 20] [--parent DIR] [--out profiles/lr_schedule_timing.json]
"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

LR = 1e-4


def build(cfg, dev, ds, B, nb, autotune, **opt_kw):
    from raindrop_amd import dp, feed, synth
    from raindrop_amd.models_rd import Raindrop_v2
    from raindrop_amd.optim import FlatAdam
    from raindrop_amd.step import TrainStep
    m = Raindrop_v2(cfg["d_inp"], cfg["d_model"], cfg["nhead"], cfg["nhid"], cfg["nlayers"], cfg["dropout"], cfg["max_len"],
                    cfg["d_static"], cfg["MAX"], 0.5, cfg["aggreg"], cfg["n_classes"], synth.make_structure(cfg, "ones"),
                    sensor_wise_mask=False)
    synth.fill_params_(m, seed=3)
    m = m.to(dev).train()
    named = dict(m.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names(cfg)], n_buckets=2)
    opt = FlatAdam(flat.flatten_parameters(), lr=LR, **opt_kw)
    out = ds.alloc(B)
    ds.batch(np.arange(B), out=out)
    fd = feed.EpochFeed(ds, B, nb)
    step = TrainStep(m, flat, dict(src=out["P"], times=out["Ptime"], static=out["Pstatic"], y=out["y"], lengths=out["lengths"]),
                     autotune=autotune, feed=fd)
    step.capture_full(opt)
    return step, opt, fd


def bench_line(tree, args):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)]
    p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise RuntimeError("bench.py in %s failed (%d): %s" % (tree, p.returncode, p.stderr[-2000:]))
    return json.loads(lines[-1])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=20, help="epochs per block (a block is epochs x n_batches steps)")
    ap.add_argument("--samples", type=int, default=3880)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py alternates between the trees")
    ap.add_argument("--bench-reps", type=int, default=6)
    ap.add_argument("--bench-steps", type=int, default=300)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lr_schedule_timing.json"))
    a = ap.parse_args(argv)
    from raindrop_amd import feed, synth
    from raindrop_amd.optim import LRSchedule
    dev = torch.device("cuda", 0)
    cfg, N, B = synth.make_config("P19"), a.samples, a.batch
    data = synth.make_batch(cfg, N, seed=1)
    y = (np.random.default_rng(2).random(N) < 0.3).astype(np.int64)          # a 30 % minority, tripled by the plan (strategy 2)
    ds = feed.DeviceDataset(data["src"], data["times"], data["static"], torch.from_numpy(y), device=dev)
    np.random.seed(0)
    planner = feed.EpochPlanner(y, batch_size=B, strategy=2, n_total=N)
    nb = int(planner.n_batches)
    steps = a.epochs * nb
    table = LRSchedule.warmup_cosine((a.blocks + 1) * steps, warmup=steps // 2, min_factor=0.01)   # one run over every block of leg b
    s_a, o_a, f_a = build(cfg, dev, ds, B, nb, True)              # the row-block masks it picks stay set: the other steps run the same
    s_b, o_b, f_b = build(cfg, dev, ds, B, nb, False, schedule=table)
    s_c, o_c, f_c = build(cfg, dev, ds, B, nb, False)
    assert tuple(o_a.step_cell.shape) == (8,) and tuple(o_b.step_cell.shape) == (8 + len(table),) and o_c.schedule is None

    def epochs(step, fd, plans, before=None):
        for plan in plans:
            fd.load_epoch(plan)
            while fd.remaining():
                if before is not None:
                    before()
                step.run_full()
            fd.history()

    def host_rate():
        o_c.lr = LR * table.factor(o_c.t + 1)
    legs = {"a_no_schedule": lambda plans: epochs(s_a, f_a, plans), "b_device_schedule": lambda plans: epochs(s_b, f_b, plans),
            "c_host_assigned": lambda plans: epochs(s_c, f_c, plans, host_rate)}
    times = {k: [] for k in legs}
    for block in range(-1, a.blocks):                            # block -1: the warm-up of every leg, not recorded
        plans = [planner.next_epoch() for _ in range(a.epochs)]
        for name, fn in legs.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn(plans)
            torch.cuda.synchronize(); t1 = time.perf_counter()
            if block >= 0:
                times[name].append((t1 - t0) * 1e3 / steps)
    want = LR * table.factor(o_b.t)
    assert o_a.t == o_b.t == o_c.t == (a.blocks + 1) * steps and o_b.current_lr() == o_c.current_lr() == want, (o_b.current_lr(), o_c.current_lr(), want)
    assert all(f.bad_indices() == 0 for f in (f_a, f_b, f_c)) and all(bool(torch.isfinite(s.loss)) for s in (s_a, s_b, s_c))
    assert s_a.captures == s_b.captures == s_c.captures == 1
    summ = {k: dict(median=round(statistics.median(v), 5), min=round(min(v), 5), max=round(max(v), 5), blocks=[round(x, 5) for x in v])
            for k, v in times.items()}
    med = {k: v["median"] for k, v in summ.items()}
    doc = {"workload": "P19, B=%d, dataset of %d samples, dropout %.1f, fwd+CE+bwd+Adam as one hipGraph (capture_full) on the epoch feed; "
                       "%d batches per epoch, %d epochs per block; schedule: warmup_cosine over %d steps (a table of %d bytes behind the "
                       "step state)" % (B, N, cfg["dropout"], nb, a.epochs, len(table), 8 * len(table)),
           "device": torch.cuda.get_device_name(0),
           "unit": "ms of wall time per step", "order": "a b c alternating, %d blocks after one warm-up block" % a.blocks,
           "legs": summ, "b_minus_a_ms": round(med["b_device_schedule"] - med["a_no_schedule"], 5),
           "c_minus_b_ms": round(med["c_host_assigned"] - med["b_device_schedule"], 5),
           "a_block_spread_ms": round(summ["a_no_schedule"]["max"] - summ["a_no_schedule"]["min"], 5),
           "final_rate": {"device": o_b.current_lr(), "host": o_c.current_lr()},
           "tuned": [s_a.tuned_rows32, s_a.tuned_waves16], "token_plan": s_a.plan is not None}
    for s in (s_a, s_b, s_c):
        s.close()
    print(json.dumps({k: doc[k] for k in ("legs", "b_minus_a_ms", "c_minus_b_ms", "a_block_spread_ms")}), flush=True)
    if a.parent:
        del s_a, s_b, s_c
        torch.cuda.empty_cache()
        runs = {"this_tree": [], "parent": []}
        for rep in range(a.bench_reps):
            order = (("this_tree", ROOT), ("parent", os.path.abspath(a.parent)))
            for name, tree in (order if rep % 2 == 0 else order[::-1]):
                runs[name].append(bench_line(tree, a))
                print(name, runs[name][-1]["ms_per_step"], flush=True)
        ms = {k: [r["ms_per_step"] for r in v] for k, v in runs.items()}
        doc["bench"] = {"command": "bench.py --gpus 1 --steps %d --warmup %d" % (a.bench_steps, a.bench_warmup),
                        "order": "this tree and the parent commit, alternating, %d processes each" % a.bench_reps, "ms_per_step": ms,
                        "median_ms_per_step": {k: statistics.median(v) for k, v in ms.items()},
                        "margin": "the parent's own process spread in this run: min .. max of its processes",
                        "parent_spread_ms": round(max(ms["parent"]) - min(ms["parent"]), 5),
                        "this_minus_parent_median_ms": round(statistics.median(ms["this_tree"]) - statistics.median(ms["parent"]), 5),
                        "inside_parents_spread": statistics.median(ms["this_tree"]) <= max(ms["parent"]),
                        "lines": {k: v[-1] for k, v in runs.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
