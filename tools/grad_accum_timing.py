"""Cost of gradient accumulation in the whole-step graph, in one process: P19, B = 256, a dataset of 3880 samples, the whole step as
hipGraphs (`capture_full`) on the epoch feed in both legs (after tools/lr_schedule_timing.py) --

  a  accumulate=1: the step as it always was, one graph, `run_full()` per batch;
  b  accumulate=4: `run_full()` per MICRO-batch -- three replays of the micro graph (feed gather, body, rd_grad_accumulate, feed
     record) and one of the closing graph (rd_grad_accumulate_close, the update) per window; an epoch's last window is closed
     where the plan ends (`close_window=True`), as `trainer.fit` does.

Wall time per micro-step (host clock around a block that ends in a device synchronise), blocks alternating a b a b ... after a warm-up
block of both legs, median / min / max over the blocks; leg b also per window (= per optimizer step).  Then the graphs' own
durations: HIP events around runs of replays of a's graph, b's micro graph and b's closing graph (the feed's plan reloaded in front of
every run, so every gather reads a real batch).  With `--parent DIR` (a built checkout of the parent commit) `bench.py` -- the
path with accumulate=1 -- is then run alternately in this tree and in DIR, `--bench-reps` times each: THE MARGIN is the parent's own
spread over its processes (min .. max), not a figure fixed here.

    python tools/grad_accum_timing.py [--blocks 7] [--epochs 20] [--parent DIR] [--out profiles/grad_accum_timing.json]
"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

LR = 1e-4
K = 4


def build(cfg, dev, ds, B, nb, autotune, **step_kw):
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
    opt = FlatAdam(flat.flatten_parameters(), lr=LR)
    out = ds.alloc(B)
    ds.batch(np.arange(B), out=out)
    fd = feed.EpochFeed(ds, B, nb)
    step = TrainStep(m, flat, dict(src=out["P"], times=out["Ptime"], static=out["Pstatic"], y=out["y"], lengths=out["lengths"]),
                     autotune=autotune, feed=fd, **step_kw)
    step.capture_full(opt)
    return step, opt, fd


def bench_line(tree, args):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)]
    p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise RuntimeError("bench.py in %s failed (%d): %s" % (tree, p.returncode, p.stderr[-2000:]))
    return json.loads(lines[-1])


def graph_ms(graph, fd, plan, runs):
    """ms per replay of `graph` by HIP events, over `runs` runs of len(plan) replays each (the plan reloaded in front of each)"""
    out = []
    for _ in range(runs):
        fd.load_epoch(plan)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in plan:
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / len(plan))
    return dict(median=round(statistics.median(out), 5), min=round(min(out), 5), max=round(max(out), 5))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=20, help="epochs per block (a block is epochs x n_batches micro-steps)")
    ap.add_argument("--samples", type=int, default=3880)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--graph-runs", type=int, default=9)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py alternates between the trees")
    ap.add_argument("--bench-reps", type=int, default=6)
    ap.add_argument("--bench-steps", type=int, default=300)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_accum_timing.json"))
    a = ap.parse_args(argv)
    from raindrop_amd import feed, synth
    from raindrop_amd.trainer import _window_plan
    dev = torch.device("cuda", 0)
    cfg, N, B = synth.make_config("P19"), a.samples, a.batch
    data = synth.make_batch(cfg, N, seed=1)
    y = (np.random.default_rng(2).random(N) < 0.3).astype(np.int64)          # a 30 % minority, tripled by the plan (strategy 2)
    ds = feed.DeviceDataset(data["src"], data["times"], data["static"], torch.from_numpy(y), device=dev)
    np.random.seed(0)
    planner = feed.EpochPlanner(y, batch_size=B, strategy=2, n_total=N)
    nb = int(planner.n_batches)
    steps, windows = a.epochs * nb, a.epochs * _window_plan(nb, K)[0]
    s_a, o_a, f_a = build(cfg, dev, ds, B, nb, True)              # the row-block masks it picks stay set: the other step runs the same
    s_b, o_b, f_b = build(cfg, dev, ds, B, nb, False, accumulate=K)
    assert s_a.acc is None and s_a.graph_full_micro is None and s_b.acc is not None and s_b.graph_full_micro is not None

    def epochs(step, fd, plans):
        for plan in plans:
            fd.load_epoch(plan)
            while fd.remaining():
                step.run_full(close_window=fd.remaining() == 1)
            fd.history()
    legs = {"a_accumulate_1": lambda plans: epochs(s_a, f_a, plans), "b_accumulate_4": lambda plans: epochs(s_b, f_b, plans)}
    times = {k: [] for k in legs}
    for block in range(-1, a.blocks):                            # block -1: the warm-up of both legs, not recorded
        plans = [planner.next_epoch() for _ in range(a.epochs)]
        for name, fn in legs.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn(plans)
            torch.cuda.synchronize(); t1 = time.perf_counter()
            if block >= 0:
                times[name].append((t1 - t0) * 1e3 / steps)
    assert o_a.t == (a.blocks + 1) * steps and o_b.t == (a.blocks + 1) * windows, (o_a.t, o_b.t)
    assert s_b.window_position() == 0 and not bool(s_b.acc.any())
    assert all(f.bad_indices() == 0 for f in (f_a, f_b)) and all(bool(torch.isfinite(s.loss)) for s in (s_a, s_b))
    assert s_a.captures == s_b.captures == 1
    summ = {k: dict(median=round(statistics.median(v), 5), min=round(min(v), 5), max=round(max(v), 5), blocks=[round(x, 5) for x in v])
            for k, v in times.items()}
    per_window = [x * steps / windows for x in times["b_accumulate_4"]]
    plan = planner.next_epoch()
    graphs = {"a_step_graph": graph_ms(s_a.graph_full, f_a, plan, a.graph_runs),
              "b_micro_graph": graph_ms(s_b.graph_full_micro, f_b, plan, a.graph_runs),
              "b_closing_graph": graph_ms(s_b.graph_full, f_b, plan, a.graph_runs)}
    med = {k: v["median"] for k, v in summ.items()}
    doc = {"workload": "P19, B=%d, dataset of %d samples, dropout %.1f, fwd+CE+bwd+Adam as hipGraphs (capture_full) on the epoch feed; "
                       "%d batches per epoch, %d epochs per block; leg b: accumulate=%d, %d optimizer steps per epoch, the last window "
                       "of %d micro-batches" % ((B, N, cfg["dropout"], nb, a.epochs, K) + _window_plan(nb, K)),
           "device": torch.cuda.get_device_name(0),
           "unit": "ms of wall time per micro-step (one batch of %d)" % B,
           "order": "a b alternating, %d blocks after one warm-up block" % a.blocks,
           "legs": summ, "b_minus_a_ms_per_micro_step": round(med["b_accumulate_4"] - med["a_accumulate_1"], 5),
           "b_ms_per_window": dict(median=round(statistics.median(per_window), 5), min=round(min(per_window), 5), max=round(max(per_window), 5)),
           "a_block_spread_ms": round(summ["a_accumulate_1"]["max"] - summ["a_accumulate_1"]["min"], 5),
           "graph_replay_ms": dict(graphs, unit="ms per replay by HIP events, %d runs of %d back-to-back replays" % (a.graph_runs, len(plan))),
           "tuned": [s_a.tuned_rows32, s_a.tuned_waves16], "token_plan": s_a.plan is not None}
    for s in (s_a, s_b):
        s.close()
    print(json.dumps({k: doc[k] for k in ("legs", "b_minus_a_ms_per_micro_step", "b_ms_per_window", "a_block_spread_ms", "graph_replay_ms")}),
          flush=True)
    if a.parent:
        del s_a, s_b
        torch.cuda.empty_cache()
        runs = {"this_tree": [], "parent": []}
        for rep in range(a.bench_reps):
            order = (("this_tree", ROOT), ("parent", os.path.abspath(a.parent)))
            for name, tree in (order if rep % 2 == 0 else order[::-1]):
                runs[name].append(bench_line(tree, a))
                print(name, runs[name][-1]["ms_per_step"], flush=True)
        ms = {k: [r["ms_per_step"] for r in v] for k, v in runs.items()}
        doc["bench"] = {"command": "bench.py --gpus 1 --steps %d --warmup %d" % (a.bench_steps, a.bench_warmup),
                        "order": "this tree (accumulate=1: the default) and the parent commit, alternating, %d processes each" % a.bench_reps,
                        "ms_per_step": ms, "median_ms_per_step": {k: statistics.median(v) for k, v in ms.items()},
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
