"""One validation pass, old path against new, same process: P19 shape, N = 3880 synthetic samples, both branches of the model.

    (A) the eager path: feed.evaluate_chunked + sigmoid + device-to-host copy + host metrics (sklearn where it is importable,
        else the numpy restatement of tests/metrics_ref.py -- the output says which): what code/Raindrop.py:345-370 does per epoch
    (B) feed.validate: captured forward per chunk, metrics on the device, one device-to-host copy
    (C) feed.validate(save_free=False): the same with the training forward and its save-for-backward buffers -- the `save_free`
        column.  Only where `validate` has the keyword: run from a tree without the inference forward the tool times A and B alone,
        which is how a parent commit is measured beside this one (the trees alternating in one call:
        profiles/infer_forward_timing.json)

Legs alternate A, B, C, A, B, C, ... `--reps` times after `--warmup` untimed rounds; each leg is timed with a device synchronisation at
both ends.  Prints one JSON document (min / median / max per leg, milliseconds); `--out FILE` also writes it there
(profiles/eval_step_timing.json is this tool's output).

    python tools/eval_timing.py --reps 9 --warmup 2 --out profiles/eval_step_timing.json
"""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raindrop_amd import _lib, feed, synth                                    # noqa: E402
from raindrop_amd.models_rd import Raindrop_v2                                # noqa: E402


def host_metrics():
    try:
        from sklearn.metrics import average_precision_score, roc_auc_score
        return "sklearn", lambda y, p: (roc_auc_score(y, p), average_precision_score(y, p))
    except ImportError:
        from tests.metrics_ref import rank_column
        return "numpy restatement (tests/metrics_ref.py)", lambda y, p: rank_column(p, y == 1)[:2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3880)
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = synth.make_config("P19")
    gs = synth.make_structure(cfg, "sparse")
    data = synth.make_batch(cfg, a.n, seed=5)
    y = np.random.default_rng(5).integers(0, 2, a.n)
    ds = feed.DeviceDataset(data["src"], data["times"], data["static"], y, device=dev)
    which, host = host_metrics()
    has_save_free = "save_free" in inspect.signature(feed.validate).parameters
    res = {"shape": "P19", "n": a.n, "chunk": a.chunk, "reps": a.reps, "warmup": a.warmup, "host_metrics": which,
           "precision": int(_lib.load().rd_get_precision()), "device": torch.cuda.get_device_name(0), "unit": "ms", "save_free_column": has_save_free, "branches": {}}
    for branch, kw in (("use_beta=False", {}), ("use_beta=True", {"use_beta": True})):
        m = Raindrop_v2(cfg["d_inp"], cfg["d_model"], cfg["nhead"], cfg["nhid"], cfg["nlayers"], cfg["dropout"], cfg["max_len"],
                        cfg["d_static"], cfg["MAX"], 0.5, cfg["aggreg"], cfg["n_classes"], gs, sensor_wise_mask=False, **kw)
        synth.fill_params_(m, seed=9)
        m = m.to(dev).train()

        def leg_a():
            out = feed.evaluate_chunked(m, ds, chunk=a.chunk)
            p = torch.sigmoid(out).cpu().numpy()
            return host(y, p[:, 1])

        def leg_b():
            v = feed.validate(m, ds, transform="sigmoid", chunk=a.chunk)
            return v["auroc"], v["auprc"]

        def leg_c():
            v = feed.validate(m, ds, transform="sigmoid", chunk=a.chunk, save_free=False)
            return v["auroc"], v["auprc"]

        legs = [("A", leg_a), ("B", leg_b)] + ([("C", leg_c)] if has_save_free else [])
        t = {name: [] for name, _ in legs}
        last = {}
        for r in range(a.warmup + a.reps):
            for name, leg in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[name] = leg()
                torch.cuda.synchronize()
                if r >= a.warmup:
                    t[name].append((time.perf_counter() - t0) * 1e3)
        steps = m._eval_steps.values()
        res["branches"][branch] = {
            "A_evaluate_chunked_host_metrics": {"min": min(t["A"]), "median": statistics.median(t["A"]), "max": max(t["A"])},
            "B_validate": {"min": min(t["B"]), "median": statistics.median(t["B"]), "max": max(t["B"])},
            "B_median_below_A_min": statistics.median(t["B"]) < min(t["A"]),
            "auroc_A_B": [float(last["A"][0]), float(last["B"][0])], "auprc_A_B": [float(last["A"][1]), float(last["B"][1])],
            "eval_steps": [{"B": s.B, "token_plan": s.plan is not None, "fused_head": bool(s.head_fused),
                            "save_free": bool(getattr(s, "infer", False)), "buffer_bytes": s.buffer_bytes()} for s in steps]}
        if has_save_free:
            res["branches"][branch]["C_validate_saving"] = {"min": min(t["C"]), "median": statistics.median(t["C"]), "max": max(t["C"])}
            res["branches"][branch]["B_equals_C"] = [float(last["B"][0]) == float(last["C"][0]), float(last["B"][1]) == float(last["C"][1])]
        del m
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(doc + "\n")


if __name__ == "__main__":
    main()
