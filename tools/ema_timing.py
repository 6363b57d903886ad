"""Cost of the weight average inside the Adam launch: TrainStep.capture_full at P19, B = 256 (the model, batch, structure and
optimizer of bench.py), one hipGraph replay per step.

Two trees alternate, one GPU process at a time: `--parent-tree DIR` (a checkout of the parent commit with its library built; this
script is what runs there, against that tree's raindrop_amd) and this tree.  Every process times blocks of `--block` replays (wall
clock around a synchronize): the parent's process `ema_decay=None` only, this tree's process `ema_decay=None` and
`ema_decay=0.999` in alternating blocks (two steps in one process, as tools/ce_criterion_timing.py).

THE MARGIN: `ema_decay=None` on the two trees must agree within the spread of the PARENT's own blocks (max - min over all of its
blocks, all of its processes); the JSON records it as "parent_block_spread_ms" next to "off_this_minus_parent_ms" and
"off_within_parent_spread".  "on_minus_off_ms" is the cost of the average, both from this tree's processes.

    python tools/ema_timing.py --parent-tree DIR [--batch 256] [--block 100] [--rounds 4] [--pairs 3] [--warmup 30]
                               [--out profiles/ema_timing.json]
"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(batch, dev, **opt_kw):
    import torch
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
    opt = FlatAdam(flat.flatten_parameters(), lr=1e-4, **opt_kw)
    ts = TrainStep(model, flat, b)
    return ts, opt


def child(a):
    """one process, one tree: blocks of replays for 'off' (and 'on' with --with-on), alternating; prints one JSON line"""
    sys.path.insert(0, a.tree)
    import torch
    import raindrop_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(raindrop_amd.__file__))) == os.path.abspath(a.tree), raindrop_amd.__file__
    dev = torch.device("cuda", 0)
    steps = {"off": build(a.batch, dev)}
    if a.with_on:
        steps["on"] = build(a.batch, dev, ema_decay=0.999)
        assert steps["on"][1].hyper()[-1] == "ema" and steps["off"][1].ema is None
    for ts, opt in steps.values():
        ts.capture_full(opt)
        for _ in range(a.warmup):
            ts.run_full()
    torch.cuda.synchronize()
    blocks = {k: [] for k in steps}
    for _ in range(a.rounds):
        for name, (ts, _) in steps.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.block):
                loss = ts.run_full()
            torch.cuda.synchronize(); t1 = time.perf_counter()
            assert bool(torch.isfinite(loss))
            blocks[name].append(round((t1 - t0) * 1e3 / a.block, 5))
    out = {"blocks": blocks, "device": torch.cuda.get_device_name(0), "p_drop": steps["off"][0].p_drop}
    if a.with_on:
        out["ema_updates"] = steps["on"][1].ema_updates()
        out["steps_on"] = steps["on"][1].t
    for ts, _ in steps.values():
        ts.close()
    print("EMA_TIMING_CHILD " + json.dumps(out), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256); ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=4); ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--parent-tree", default=None); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_timing.json"))
    ap.add_argument("--child", action="store_true"); ap.add_argument("--tree", default=ROOT); ap.add_argument("--with-on", action="store_true")
    a = ap.parse_args(argv)
    if a.child:
        return child(a)
    if not a.parent_tree or not os.path.isdir(os.path.join(a.parent_tree, "raindrop_amd")):
        sys.exit("ema_timing: --parent-tree DIR (a built checkout of the parent commit) is required: the off path is measured against it")

    def run(tree, with_on):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", os.path.abspath(tree), "--batch", str(a.batch),
               "--block", str(a.block), "--rounds", str(a.rounds), "--warmup", str(a.warmup)] + (["--with-on"] if with_on else [])
        env = dict(os.environ)
        env.pop("RD_LIB_PATH", None)
        res = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=tree, timeout=400)
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("EMA_TIMING_CHILD ")]
        if res.returncode != 0 or not line:
            sys.exit("ema_timing: the process on %s failed (%d):\n%s\n%s" % (tree, res.returncode, res.stdout[-2000:], res.stderr[-4000:]))
        return json.loads(line[-1][len("EMA_TIMING_CHILD "):])

    parent, this_off, this_on, dev, info = [], [], [], None, {}
    for pair in range(a.pairs):
        order = [("parent", a.parent_tree), ("this", ROOT)] if pair % 2 == 0 else [("this", ROOT), ("parent", a.parent_tree)]
        for name, tree in order:
            r = run(tree, name == "this")
            dev = r["device"]
            if name == "parent":
                parent.append(r["blocks"]["off"])
            else:
                this_off.append(r["blocks"]["off"]); this_on.append(r["blocks"]["on"])
                info = {"ema_updates": r["ema_updates"], "steps_on": r["steps_on"], "p_drop": r["p_drop"]}
            print(name, r["blocks"], flush=True)
    flat = lambda xs: [x for run_ in xs for x in run_]
    mean = lambda xs: sum(xs) / len(xs)
    spread = round(max(flat(parent)) - min(flat(parent)), 5)
    d_off = round(mean(flat(this_off)) - mean(flat(parent)), 5)
    res = {"workload": "TrainStep.capture_full(FlatAdam(lr=1e-4)), P19 all-ones structure, B=%d, dropout %.1f, one hipGraph replay per "
                       "step; off: ema_decay=None (parent tree and this tree, one process each, alternating), on: ema_decay=0.999 "
                       "(this tree, in the off process, alternating blocks)" % (a.batch, info["p_drop"]),
           "block_steps": a.block, "rounds_per_process": a.rounds, "process_pairs": a.pairs, "warmup": a.warmup, "device": dev,
           "ms_per_step_blocks": {"parent_off": parent, "this_off": this_off, "this_on": this_on},
           "ms_per_step_mean": {"parent_off": round(mean(flat(parent)), 5), "this_off": round(mean(flat(this_off)), 5),
                                "this_on": round(mean(flat(this_on)), 5)},
           "margin": "off on the two trees must agree within the spread (max - min) of the parent's own blocks",
           "parent_block_spread_ms": spread, "off_this_minus_parent_ms": d_off, "off_within_parent_spread": abs(d_off) <= spread,
           "this_off_block_spread_ms": round(max(flat(this_off)) - min(flat(this_off)), 5),
           "on_minus_off_ms": round(mean(flat(this_on)) - mean(flat(this_off)), 5),
           "on_minus_off_ms_per_process": [round(mean(n) - mean(f), 5) for n, f in zip(this_on, this_off)],
           "ema_updates_last_process": info["ema_updates"], "steps_on_last_process": info["steps_on"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
