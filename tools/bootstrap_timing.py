"""Bootstrap confidence intervals of the validation metrics, timed in ONE process on one box:

  (a) `metrics.rank_bootstrap` at N = 3880, C = 2, R = 1000 (P19's evaluation split) with its workspace and outputs allocated once,
      wall time around a block of calls that ends in a device synchronise, against the host baseline it replaces: a device-to-host
      copy of the scores and a loop over the SAME resamples (tests/bootstrap_ref.py's draws) through sklearn's roc_auc_score /
      average_precision_score on the expanded resample (numpy sorts of tests/metrics_ref.py where sklearn is not installed), then
      numpy.percentile.  Blocks alternate between the two after one warm-up block; median / min / max over the blocks.
  (b) `feed.validate(bootstrap=None)` of this tree against a built checkout of the PARENT commit (`--parent DIR`): alternating child
      processes, each timing validate on a P19 model and a 3880-sample split; "no cost" = this tree's median inside the parent's own
      spread.  Without --parent the document says "not measured".  `validate(bootstrap=1000)` of this tree is timed beside them.

    python tools/bootstrap_timing.py [--blocks 7] [--parent DIR] [--out profiles/bootstrap_metrics_timing.json]
"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), blocks=[round(x, 4) for x in v])


def validate_child(tree, n, reps, bootstrap):
    """median ms of feed.validate on a P19 model and an n-sample split, in the tree `tree` (this process imports nothing else)"""
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    from raindrop_amd import feed, synth
    from raindrop_amd.models_rd import Raindrop_v2
    dev = torch.device("cuda", 0)
    cfg = synth.make_config("P19")
    gs = synth.make_structure(cfg, "sparse")
    model = Raindrop_v2(cfg["d_inp"], cfg["d_model"], cfg["nhead"], cfg["nhid"], cfg["nlayers"], 0.0, cfg["max_len"], cfg["d_static"],
                        cfg["MAX"], 0.5, cfg["aggreg"], cfg["n_classes"], gs, sensor_wise_mask=False)
    synth.fill_params_(model, seed=9)
    model = model.to(dev).eval()
    data = synth.make_batch(cfg, n, seed=1)
    y = (np.random.default_rng(2).random(n) < 0.04).astype(np.int64)
    ds = feed.DeviceDataset(data["src"], data["times"], data["static"], torch.from_numpy(y), device=dev)
    kw = {} if bootstrap is None else dict(bootstrap=bootstrap)
    for _ in range(3):
        v = feed.validate(model, ds, **kw)
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        v = feed.validate(model, ds, **kw)
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(ms=statistics.median(ms), auroc=v["auroc"], auroc_ci=v.get("auroc_ci"))))


def child_line(tree, a, bootstrap=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--validate-child", tree, "--samples", str(a.samples), "--reps", str(a.reps)]
    if bootstrap is not None:
        cmd += ["--child-bootstrap", str(bootstrap)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=tree)
    if out.returncode != 0:
        raise RuntimeError("child failed in %s:\n%s" % (tree, out.stderr[-2000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10, help="device calls per block")
    ap.add_argument("--samples", type=int, default=3880)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--resamples", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=15, help="validate calls a child times")
    ap.add_argument("--processes", type=int, default=4, help="child processes per tree")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--validate-child", default=None, metavar="TREE")
    ap.add_argument("--child-bootstrap", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bootstrap_metrics_timing.json"))
    a = ap.parse_args(argv)
    if a.validate_child:
        return validate_child(os.path.abspath(a.validate_child), a.samples, a.reps, a.child_bootstrap)
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from raindrop_amd import build as rd_build, metrics
    from tests import bootstrap_ref as B
    from tests import metrics_ref as M
    try:
        from sklearn.metrics import average_precision_score, roc_auc_score
        host_kind = "sklearn roc_auc_score / average_precision_score on the expanded resample"
    except ImportError:
        roc_auc_score = None
        host_kind = "numpy (tests/metrics_ref.rank_metrics_ref) on the expanded resample: sklearn is not installed"
    N, C, R, seed = a.samples, a.classes, a.resamples, 11
    s, y = M.make_case("binary" if C == 2 else "sigmoid8", N, C, 5, 0.04, 0)
    sd, yd = torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda()
    ws = metrics.bootstrap_workspace(N, C, R, sd.device)
    out = metrics.rank_bootstrap(sd, yd, n_boot=R, seed=seed, workspace=ws)
    torch.cuda.synchronize()

    def device_ms():
        t0 = time.perf_counter()
        for _ in range(a.calls):
            metrics.rank_bootstrap(sd, yd, n_boot=R, seed=seed, out=out, workspace=ws)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.calls

    def host_ms():
        t0 = time.perf_counter()
        sh, yh = sd.cpu().numpy(), yd.cpu().numpy()
        au, ap = np.full((R, C), np.nan), np.zeros((R, C))
        for r in range(R):
            idx = B.draw_indices(seed, r, N)
            if roc_auc_score is None:
                e = M.rank_metrics_ref(sh[idx], yh[idx])
                au[r], ap[r] = e["auroc"], e["auprc"]
                continue
            for c in range(C):
                t = yh[idx] == c
                if t.any():
                    ap[r, c] = average_precision_score(t, sh[idx, c])
                    if not t.all():
                        au[r, c] = roc_auc_score(t, sh[idx, c])
        ci = [np.percentile(v[~np.isnan(v)], [2.5, 97.5]) for v in (au[:, C - 1], ap[:, C - 1])]
        return (time.perf_counter() - t0) * 1e3, ci
    dev_t, host_t, ci = [], [], None
    for block in range(-1, a.blocks):
        d = device_ms()
        h, ci = host_ms()
        if block >= 0:
            dev_t.append(d); host_t.append(h)
    got = out["summary"].cpu().numpy()
    usage = {k: {f: u.get(f) for f in ("vgprs", "sgprs", "scratch", "lds", "occupancy")} for k, u in rd_build.resource_usage().items() if "k_boot" in k}
    doc = {"workload": "scores float32 [%d, %d], %d resamples, 4 %% positives; one process, one box, wall time" % (N, C, R),
           "order": "device block (%d calls, one synchronise), host block (one pass), alternating, %d blocks after one warm-up block" % (a.calls, a.blocks),
           "rank_bootstrap_ms_per_call": summary(dev_t), "host_baseline_ms": dict(summary(host_t), what="device-to-host copy + " + host_kind + " + numpy.percentile"),
           "speedup_of_medians": round(statistics.median(host_t) / statistics.median(dev_t), 1),
           "interval_of_the_last_column": {"device": [got[0, C - 1, 3:].tolist(), got[1, C - 1, 3:].tolist()], "host": [c.tolist() for c in ci]},
           "kernel_resources": usage, "validate_bootstrap_none_vs_parent": "not measured (needs --parent: a built checkout of the parent commit)"}
    print(json.dumps({k: doc[k] for k in ("rank_bootstrap_ms_per_call", "host_baseline_ms", "speedup_of_medians")}), flush=True)
    if a.parent:
        del out, ws, sd, yd
        torch.cuda.empty_cache()
        runs = {"this_tree": [], "parent": [], "this_tree_bootstrap_%d" % R: []}
        for _ in range(a.processes):
            runs["this_tree"].append(child_line(ROOT, a))
            runs["parent"].append(child_line(os.path.abspath(a.parent), a))
            runs["this_tree_bootstrap_%d" % R].append(child_line(ROOT, a, bootstrap=R))
        ms = {k: [round(r["ms"], 4) for r in v] for k, v in runs.items()}
        doc["validate_bootstrap_none_vs_parent"] = {
            "what": "median ms of feed.validate (P19 model, %d samples, one chunk pair) over %d calls per child process" % (N, a.reps),
            "order": "this tree, parent, this tree with bootstrap=%d: alternating processes, %d each" % (R, a.processes), "ms": ms,
            "median_ms": {k: statistics.median(v) for k, v in ms.items()},
            "same_auroc": len({r["auroc"] for r in runs["this_tree"] + runs["parent"]}) == 1,
            "inside_parents_spread": min(ms["parent"]) <= statistics.median(ms["this_tree"]) <= max(ms["parent"])}
        print(json.dumps(doc["validate_bootstrap_none_vs_parent"]["median_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
