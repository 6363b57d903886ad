"""Train-time augmentation inside the epoch feed, timed in ONE process at P19, B = 256 (a dataset of 3880 samples):

  kernel  the gather launch alone, by HIP events around replays of a hipGraph of 20 launches: rd_feed_gather (the yardstick of this
          run) and rd_feed_gather_aug with all rates 0, each rate alone (p_time=0.1, p_sensor=0.2, p_obs=0.1, value_noise=0.05) and
          all four together; blocks alternating over the variants after one warm-up block, median / min / max;
  step    the fed whole step (`capture_full`), wall time per step around a block that ends in a device synchronise: a feed with
          augment=None against an augmenting feed whose rates `set_augment` changes between blocks (no new capture), same
          alternation;
  regs    registers / LDS / scratch of the two instantiations of k_gather_aug and of the plain kernels, from the build's
          kernel-resource-usage records (tools/kres.py prints the same figures for one file).

The comparison of augment=None against the PARENT commit needs a built checkout of the parent: `--parent DIR` alternates bench.py
between the trees like tools/feed_graph_timing.py; without it the document says "not measured".

    python tools/feed_aug_timing.py [--blocks 7] [--epochs 20] [--parent DIR] [--out profiles/feed_aug_timing.json]
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

VARIANTS = {"aug_all_zero": {}, "p_time_0.1": dict(p_time=0.1), "p_sensor_0.2": dict(p_sensor=0.2), "p_obs_0.1": dict(p_obs=0.1),
            "value_noise_0.05": dict(value_noise=0.05), "all_four": dict(p_time=0.1, p_sensor=0.2, p_obs=0.1, value_noise=0.05)}
OFF = dict(p_time=0.0, p_sensor=0.0, p_obs=0.0, value_noise=0.0)


def summary(v):
    return dict(median=round(statistics.median(v), 5), min=round(min(v), 5), max=round(max(v), 5), blocks=[round(x, 5) for x in v])


def gather_graph(fd, batch, launches=20):
    """a hipGraph of `launches` gathers of the feed's current batch (nothing records, so the cursor stays)"""
    for _ in range(3):
        fd.enqueue_gather(batch)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fd.enqueue_gather(batch)
    g.replay()
    torch.cuda.synchronize()
    return g


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=20, help="epochs per block of the step timing")
    ap.add_argument("--samples", type=int, default=3880)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--bench-reps", type=int, default=8)
    ap.add_argument("--bench-steps", type=int, default=300)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--bench-args", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_aug_timing.json"))
    a = ap.parse_args(argv)
    import feed_graph_timing as fgt
    from raindrop_amd import build as rd_build, feed, synth
    dev = torch.device("cuda", 0)
    cfg, N, B = synth.make_config("P19"), a.samples, a.batch
    data = synth.make_batch(cfg, N, seed=1)
    y = (np.random.default_rng(2).random(N) < 0.3).astype(np.int64)
    ds = feed.DeviceDataset(data["src"], data["times"], data["static"], torch.from_numpy(y), device=dev)
    np.random.seed(0)
    planner = feed.EpochPlanner(y, batch_size=B, strategy=2, n_total=N)
    nb = int(planner.n_batches)
    fd_plain, fd_aug = feed.EpochFeed(ds, B, nb), feed.EpochFeed(ds, B, nb, augment=feed.Augment(seed=5))
    out_p, out_a = ds.alloc(B), ds.alloc(B)
    for o in (out_p, out_a):
        ds.batch(np.arange(B), out=o)
    T, W = cfg["max_len"], 2 * cfg["d_inp"]
    nbytes = 2 * B * T * (W + 1) * 4 + B * (T * 4 + 2 * cfg["d_static"] * 4 + 24)

    # ---- kernel: the gather launch alone ------------------------------------------------------------------------------------------
    plan = planner.next_epoch()
    fd_plain.load_epoch(plan); fd_aug.load_epoch(plan)
    bt = lambda o: dict(src=o["P"], times=o["Ptime"], static=o["Pstatic"], y=o["y"], lengths=o["lengths"])
    g_plain, g_aug = gather_graph(fd_plain, bt(out_p)), gather_graph(fd_aug, bt(out_a))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def gather_us(g, reps=25):
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (reps * 20) * 1e3
    ktimes = {k: [] for k in ["plain"] + list(VARIANTS)}
    for block in range(-1, a.blocks):
        for name in ktimes:
            if name != "plain":
                fd_aug.set_augment(**dict(OFF, **VARIANTS[name]))
            us = gather_us(g_plain if name == "plain" else g_aug)
            if block >= 0:
                ktimes[name].append(us)
    kernel = {k: dict(summary(v), GBps=round(nbytes / statistics.median(v) / 1e3, 1)) for k, v in ktimes.items()}
    print(json.dumps({k: v["median"] for k, v in kernel.items()}), flush=True)

    # ---- step: the fed whole step ---------------------------------------------------------------------------------------------------
    plain = fgt.build(cfg, dev, fd_plain, out_p, autotune=True)
    auged = fgt.build(cfg, dev, fd_aug, out_a, autotune=False)
    captures = auged.captures
    steps = a.epochs * nb

    def leg(step, fd, plans):
        for p in plans:
            fd.load_epoch(p)
            while fd.remaining():
                step.run_full()
            fd.history()
    stimes = {k: [] for k in ["augment_none"] + list(VARIANTS)}
    for block in range(-1, a.blocks):
        for name in stimes:
            plans = [planner.next_epoch() for _ in range(a.epochs)]
            if name != "augment_none":
                fd_aug.set_augment(**dict(OFF, **VARIANTS[name]))
            torch.cuda.synchronize(); t0 = time.perf_counter()
            leg(plain, fd_plain, plans) if name == "augment_none" else leg(auged, fd_aug, plans)
            torch.cuda.synchronize(); t1 = time.perf_counter()
            if block >= 0:
                stimes[name].append((t1 - t0) * 1e3 / steps)
    assert auged.captures == captures and fd_plain.bad_indices() == 0 and fd_aug.bad_indices() == 0
    assert bool(torch.isfinite(plain.loss)) and bool(torch.isfinite(auged.loss))
    step = {k: summary(v) for k, v in stimes.items()}
    print(json.dumps({k: v["median"] for k, v in step.items()}), flush=True)
    tuned = [plain.tuned_rows32, plain.tuned_waves16]
    plain.close(); auged.close()

    usage = {k: {f: u.get(f) for f in ("vgprs", "agprs", "sgprs", "scratch", "lds", "occupancy")} for k, u in rd_build.resource_usage().items()
             if any(n in k for n in ("k_gather_aug", "k_feed_gather", "k_batch_gather"))}
    doc = {"workload": "P19, B=%d, dataset of %d samples, %d batches per epoch; one process, one box" % (B, N, nb),
           "kernel": {"unit": "us per gather launch (HIP events around 25 replays of a hipGraph of 20 launches)", "bytes_per_batch": nbytes,
                      "order": "plain and the augmenting variants alternating, %d blocks after one warm-up block" % a.blocks, "variants": kernel},
           "step": {"unit": "ms of wall time per fed capture_full step, %d epochs per block" % a.epochs,
                    "order": "augment=None and the variants (set_augment, no new capture) alternating, %d blocks after one warm-up block" % a.blocks,
                    "variants": step, "tuned": tuned},
           "kernel_resources": usage,
           "augment_none_vs_parent": "not measured (needs --parent: a built checkout of the parent commit)"}
    if a.parent:
        del plain, auged
        torch.cuda.empty_cache()
        runs = {"this_tree": [], "parent": []}
        for _ in range(a.bench_reps):
            for name, tree in (("this_tree", ROOT), ("parent", os.path.abspath(a.parent))):
                runs[name].append(fgt.bench_line(tree, a))
        ms = {k: [r["ms_per_step"] for r in v] for k, v in runs.items()}
        doc["augment_none_vs_parent"] = {"command": "bench.py --gpus 1 --steps %d --warmup %d %s" % (a.bench_steps, a.bench_warmup, a.bench_args),
                                         "order": "this tree, parent, alternating processes, %d times each" % a.bench_reps, "ms_per_step": ms,
                                         "median_ms_per_step": {k: statistics.median(v) for k, v in ms.items()},
                                         "inside_parents_spread": min(ms["parent"]) <= statistics.median(ms["this_tree"]) <= max(ms["parent"])}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
