"""Calibration on the device, timed on one box; nothing here is gated, the numbers are written down:

  (a) `metrics.fit_temperature` + `metrics.calibration(n_bins=15, temperature=<the fit's tensor>)` at N = 3880 with C = 2 and C = 8,
      outputs and workspace allocated once, wall time around a block of calls that ends in a device synchronise, against what it
      replaces: a device-to-host copy of the logits and the numpy reference there (tests/calibration_ref.py: fit by bisection, then
      the statistics).  Blocks alternate between the two after one warm-up block; median / min / max over the blocks.
  (b) `feed.validate(calibration=None)` of this tree against a built checkout of the PARENT commit (`--parent DIR`): alternating child
      processes, each timing validate on a P19 model and a 3880-sample split; both medians and the parent's spread are reported,
      nothing is asserted.  Without --parent the document says "not measured".
  (c) `feed.validate(calibration=15, temperature="fit")` of this tree, in child processes beside those of (b).

    python tools/calibration_timing.py [--blocks 7] [--parent DIR] [--out profiles/calibration_timing.json]
"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), blocks=[round(x, 4) for x in v])


def validate_child(tree, n, reps, kw):
    """median ms of feed.validate(**kw) on a P19 model and an n-sample split, in the tree `tree` (this process imports nothing else)"""
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
    for _ in range(3):
        v = feed.validate(model, ds, **kw)
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        v = feed.validate(model, ds, **kw)
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(ms=statistics.median(ms), auroc=v["auroc"], ece=v.get("ece"), temperature=v.get("temperature"),
                          temperature_status=v.get("temperature_status"))))


def child_line(tree, a, kw):
    cmd = [sys.executable, os.path.abspath(__file__), "--validate-child", tree, "--samples", str(a.samples), "--reps", str(a.reps),
           "--child-kw", json.dumps(kw)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=tree)
    if out.returncode != 0:
        raise RuntimeError("child failed in %s:\n%s" % (tree, out.stderr[-2000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="device calls per block")
    ap.add_argument("--samples", type=int, default=3880)
    ap.add_argument("--bins", type=int, default=15)
    ap.add_argument("--reps", type=int, default=15, help="validate calls a child times")
    ap.add_argument("--processes", type=int, default=4, help="child processes per tree")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--validate-child", default=None, metavar="TREE")
    ap.add_argument("--child-kw", default="{}")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibration_timing.json"))
    a = ap.parse_args(argv)
    if a.validate_child:
        return validate_child(os.path.abspath(a.validate_child), a.samples, a.reps, json.loads(a.child_kw))
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from raindrop_amd import build as rd_build, metrics
    from tests import calibration_ref as K
    N, M = a.samples, a.bins
    usage = {k: {f: u.get(f) for f in ("vgprs", "sgprs", "scratch", "lds", "occupancy")} for k, u in rd_build.resource_usage().items()
             if "k_calib" in k or "k_fit_temperature" in k}
    doc = {"workload": "logits float32 [%d, C], labels drawn from softmax(logits / 1.7), %d bins; one process, one box, wall time" % (N, M),
           "order": "device block (%d calls of fit_temperature + calibration, one synchronise), host block (one pass), alternating, %d blocks "
                    "after one warm-up block" % (a.calls, a.blocks), "fit_plus_calibration": {}, "kernel_resources": usage,
           "validate_calibration_none_vs_parent": "not measured (needs --parent: a built checkout of the parent commit)",
           "validate_calibration_fit": "not measured (needs --parent: timed beside it)"}
    for C in (2, 8):
        lg, y = K.make_logits(31 + C, N, C, 1.7)
        ld, yd = torch.from_numpy(lg).cuda(), torch.from_numpy(y).cuda()
        ws = metrics.calibration_workspace(N, C, M, ld.device)
        column = 1 if C == 2 else None
        fit = metrics.fit_temperature(ld, yd)
        out = metrics.calibration(ld, yd, n_bins=M, temperature=fit["result"], column=column, workspace=ws)
        torch.cuda.synchronize()

        def device_ms():
            t0 = time.perf_counter()
            for _ in range(a.calls):
                metrics.fit_temperature(ld, yd, out=fit)
                metrics.calibration(ld, yd, n_bins=M, temperature=fit["result"], column=column, out=out, workspace=ws)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / a.calls

        def host_ms():
            t0 = time.perf_counter()
            lh, yh = ld.cpu().numpy(), yd.cpu().numpy()
            f = K.fit_ref(lh, yh)
            r = K.calibration_ref(lh, yh, M, f["T"], column)
            return (time.perf_counter() - t0) * 1e3, f, r
        dev_t, host_t = [], []
        for block in range(-1, a.blocks):
            d = device_ms()
            h, f, r = host_ms()
            if block >= 0:
                dev_t.append(d); host_t.append(h)
        res = fit["result"].cpu().numpy()
        doc["fit_plus_calibration"]["C=%d" % C] = {
            "device_ms_per_call": summary(dev_t), "host_baseline_ms": dict(summary(host_t), what="device-to-host copy + numpy fit by bisection + numpy statistics"),
            "ratio_of_medians": round(statistics.median(host_t) / statistics.median(dev_t), 1),
            "temperature": {"device": float(res[0]), "host": f["T"]}, "evaluations": int(res[4]), "status": int(res[5]),
            "ece": {"device": float(out["ece"].item()), "host": float(r["summary"][0])}}
        print(json.dumps({"C": C, "device_ms": statistics.median(dev_t), "host_ms": statistics.median(host_t)}), flush=True)
        del out, ws, ld, yd, fit
    if a.parent:
        torch.cuda.empty_cache()
        kw_fit = dict(calibration=M, temperature="fit")
        runs = {"this_tree": [], "parent": [], "this_tree_calibration_fit": []}
        for _ in range(a.processes):
            runs["this_tree"].append(child_line(ROOT, a, {}))
            runs["parent"].append(child_line(os.path.abspath(a.parent), a, {}))
            runs["this_tree_calibration_fit"].append(child_line(ROOT, a, kw_fit))
        ms = {k: [round(r["ms"], 4) for r in v] for k, v in runs.items()}
        doc["validate_calibration_none_vs_parent"] = {
            "what": "median ms of feed.validate (P19 model, %d samples) over %d calls per child process; reported, not asserted" % (N, a.reps),
            "order": "this tree, parent, this tree with calibration=%d temperature='fit': alternating processes, %d each" % (M, a.processes),
            "ms": {k: ms[k] for k in ("this_tree", "parent")},
            "median_ms": {k: statistics.median(ms[k]) for k in ("this_tree", "parent")},
            "parent_spread_ms": [min(ms["parent"]), max(ms["parent"])],
            "same_auroc": len({r["auroc"] for r in runs["this_tree"] + runs["parent"]}) == 1,
            "inside_parents_spread": min(ms["parent"]) <= statistics.median(ms["this_tree"]) <= max(ms["parent"])}
        last = runs["this_tree_calibration_fit"][-1]
        doc["validate_calibration_fit"] = {"ms": ms["this_tree_calibration_fit"], "median_ms": statistics.median(ms["this_tree_calibration_fit"]),
                                           "temperature": last["temperature"], "temperature_status": last["temperature_status"], "ece": last["ece"]}
        print(json.dumps({"validate_ms": doc["validate_calibration_none_vs_parent"]["median_ms"],
                          "with_fit": doc["validate_calibration_fit"]["median_ms"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
