"""Host side of a training step with and without the epoch feed, in one process: P19, B = 256, a dataset of 3880 samples, the
whole step as one hipGraph (`capture_full`) in all three legs --

  A  the hand-fed step: a host index vector, `ds.batch(idx, out=)` (a pageable host-to-device copy + rd_batch_gather), `run_full()`;
  B  the fed step: `EpochFeed.load_epoch` once per epoch, `run_full()` per batch, `history()` once per epoch;
  C  `run_full()` on resident inputs (what bench.py times): the floor.

Wall time per step (host clock around a block that ends in a device synchronise), blocks alternating A B C A B C ... after a
warm-up of every leg, median / min / max over the blocks; B - A and B - C from the medians, to be read against the legs' own
spread.  A and B draw the same plans (`EpochPlanner`, strategy 2, planned in front of the clock).  With `--parent DIR` (a built
checkout of the parent commit) `bench.py` is then run alternately in this tree and in DIR, `--bench-reps` times each, and both
trees' lines go into the document: the step without a feed must stay inside the parent's own spread.

    python tools/feed_graph_timing.py [--blocks 7] [--epochs 50] [--parent DIR] [--out profiles/feed_graph_timing.json]
"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch


def build(cfg, dev, feed_obj, out, autotune):
    from raindrop_amd import dp, synth
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
    opt = FlatAdam(flat.flatten_parameters(), lr=1e-4)
    batch = dict(src=out["P"], times=out["Ptime"], static=out["Pstatic"], y=out["y"], lengths=out["lengths"])
    step = TrainStep(m, flat, batch, autotune=autotune, feed=feed_obj)
    step.capture_full(opt)
    return step


def bench_line(tree, args):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)] + args.bench_args.split()
    p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise RuntimeError("bench.py in %s failed (%d): %s" % (tree, p.returncode, p.stderr[-2000:]))
    return json.loads(lines[-1])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=50, help="epochs per block (a block is epochs x n_batches steps)")
    ap.add_argument("--samples", type=int, default=3880)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py alternates between the trees")
    ap.add_argument("--bench-reps", type=int, default=8)
    ap.add_argument("--bench-steps", type=int, default=300)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--bench-args", default="", help="further bench.py arguments, one string")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_graph_timing.json"))
    a = ap.parse_args(argv)
    from raindrop_amd import feed, synth
    dev = torch.device("cuda", 0)
    cfg, N, B = synth.make_config("P19"), a.samples, a.batch
    data = synth.make_batch(cfg, N, seed=1)
    y = (np.random.default_rng(2).random(N) < 0.3).astype(np.int64)          # a 30 % minority, tripled by the plan (strategy 2)
    ds = feed.DeviceDataset(data["src"], data["times"], data["static"], torch.from_numpy(y), device=dev)
    np.random.seed(0)
    planner = feed.EpochPlanner(y, batch_size=B, strategy=2, n_total=N)
    nb = int(planner.n_batches)
    fd = feed.EpochFeed(ds, B, nb)
    out_a, out_b = ds.alloc(B), ds.alloc(B)
    for o in (out_a, out_b):
        ds.batch(np.arange(B), out=o)
    hand = build(cfg, dev, None, out_a, autotune=True)           # the row-block masks it picks stay set: the second step runs the same
    fed = build(cfg, dev, fd, out_b, autotune=False)
    steps = a.epochs * nb

    def leg_a(plans):
        for plan in plans:
            for idx in plan:
                ds.batch(idx, out=out_a)
                hand.run_full()

    def leg_b(plans):
        for plan in plans:
            fd.load_epoch(plan)
            while fd.remaining():
                fed.run_full()
            fd.history()

    def leg_c(plans):
        for _ in range(steps):
            hand.run_full()
    legs = {"A_hand_fed": leg_a, "B_fed": leg_b, "C_resident": leg_c}
    times = {k: [] for k in legs}
    for block in range(-1, a.blocks):                            # block -1: the warm-up of every leg, not recorded
        for name, fn in legs.items():
            plans = [planner.next_epoch() for _ in range(a.epochs)]
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn(plans)
            torch.cuda.synchronize(); t1 = time.perf_counter()
            if block >= 0:
                times[name].append((t1 - t0) * 1e3 / steps)
    assert fd.bad_indices() == 0 and bool(torch.isfinite(hand.loss)) and bool(torch.isfinite(fed.loss))
    summ = {k: dict(median=round(statistics.median(v), 5), min=round(min(v), 5), max=round(max(v), 5), blocks=[round(x, 5) for x in v])
            for k, v in times.items()}
    doc = {"workload": "P19, B=%d, dataset of %d samples, dropout %.1f, fwd+CE+bwd+Adam as one hipGraph (capture_full); %d batches "
                       "per epoch, %d epochs per block" % (B, N, cfg["dropout"], nb, a.epochs),
           "unit": "ms of wall time per step", "order": "A B C alternating, %d blocks after one warm-up block" % a.blocks,
           "legs": summ, "B_minus_A_ms": round(summ["B_fed"]["median"] - summ["A_hand_fed"]["median"], 5),
           "B_minus_C_ms": round(summ["B_fed"]["median"] - summ["C_resident"]["median"], 5),
           "tuned": [hand.tuned_rows32, hand.tuned_waves16], "token_plan": hand.plan is not None}
    hand.close(); fed.close()
    print(json.dumps({k: doc[k] for k in ("legs", "B_minus_A_ms", "B_minus_C_ms")}), flush=True)
    if a.parent:
        del hand, fed
        torch.cuda.empty_cache()
        runs = {"this_tree": [], "parent": []}
        for _ in range(a.bench_reps):
            for name, tree in (("this_tree", ROOT), ("parent", os.path.abspath(a.parent))):
                runs[name].append(bench_line(tree, a))
                print(name, runs[name][-1]["ms_per_step"], flush=True)
        ms = {k: [r["ms_per_step"] for r in v] for k, v in runs.items()}
        tuned = {k: [[r["config"].get("tuned", {}).get(n) for n in ("rowgemm_rows32", "rowgemm_waves16")] for r in v] for k, v in runs.items()}
        doc["bench"] = {"command": "bench.py --gpus 1 --steps %d --warmup %d %s" % (a.bench_steps, a.bench_warmup, a.bench_args),
                        "order": "this tree, parent, alternating, %d times each" % a.bench_reps, "ms_per_step": ms, "tuned": tuned,
                        "median_ms_per_step": {k: statistics.median(v) for k, v in ms.items()},
                        "inside_parents_spread": min(ms["parent"]) <= statistics.median(ms["this_tree"]) <= max(ms["parent"]),
                        "lines": {k: v[-1] for k, v in runs.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
