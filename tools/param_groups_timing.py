"""Cost of parameter groups inside the Adam launch: TrainStep.capture_full at P19, B = 256 (the model, batch, structure and
optimizer of bench.py, with weight_decay = 0.01), one hipGraph replay per step.  After tools/ema_timing.py.

Two trees alternate, one GPU process at a time: `--parent-tree DIR` (a checkout of the parent commit with its library built; this
script is what runs there, against that tree's raindrop_amd) and this tree.  Every process times blocks of `--block` replays (wall
clock around a synchronize): the parent's process groups off only, this tree's process groups off and `optim.no_decay` groups on in
alternating blocks.  This tree's process then times THE UPDATE LAUNCH ALONE: one hipGraph of 100 x `step_captured()` per
optimizer (grouped and plain, on the step's own flat buffers), HIP events around a replay, alternating.

THE MARGIN: groups off on the two trees must agree within the spread of the PARENT's own blocks (max - min over all of its blocks,
all of its processes): "parent_block_spread_ms", "off_this_minus_parent_ms", "off_within_parent_spread".  "on_minus_off_ms" is the
cost of the byte map and the cell rows on the step, "update_launch_us" the launch alone -- both from this tree's processes.

    python tools/param_groups_timing.py --parent-tree DIR [--batch 256] [--block 100] [--rounds 4] [--pairs 3] [--warmup 30]
                                        [--out profiles/param_groups_timing.json]
"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WD = 0.01


def build(batch, dev, grouped):
    import torch
    from raindrop_amd import dp, optim, synth
    from raindrop_amd.models_rd import Raindrop_v2
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
    kw = dict(groups=optim.ParamGroups(flat, [optim.no_decay(flat)])) if grouped else {}
    opt = optim.FlatAdam(flat.flatten_parameters(), lr=1e-4, weight_decay=WD, **kw)
    ts = TrainStep(model, flat, b)
    return ts, opt


def update_alone(opts, reps, rounds):
    """us per update launch: per optimizer ONE hipGraph of `reps` x step_captured() (advance launch included, the same one in both),
    HIP events around a replay, `rounds` alternating replays each"""
    import torch
    from raindrop_amd.step import capture_graphs
    graphs = {}
    for name, opt in opts.items():
        def body(opt=opt):
            for _ in range(reps):
                opt.step_captured()
        graphs[name], = capture_graphs([body])
    out = {k: [] for k in opts}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); g.replay(); e1.record()
            torch.cuda.synchronize()
            out[name].append(round(e0.elapsed_time(e1) * 1e3 / reps, 4))
    return out


def child(a):
    """one process, one tree: blocks of replays for 'off' (and 'on' with --with-on), alternating; prints one JSON line"""
    sys.path.insert(0, a.tree)
    import torch
    import raindrop_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(raindrop_amd.__file__))) == os.path.abspath(a.tree), raindrop_amd.__file__
    dev = torch.device("cuda", 0)
    steps = {"off": build(a.batch, dev, False)}
    if a.with_on:
        steps["on"] = build(a.batch, dev, True)
        assert steps["on"][1].hyper()[-1] == "grp" and steps["off"][1].hyper()[-1] != "grp"
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
        info = steps["on"][1].group_info()
        out["groups"] = [dict(tensors=len(g["names"]), lr_scale=g["lr_scale"], weight_decay=g["weight_decay"]) for g in info]
        out["n"] = steps["on"][1].param.numel()
        out["update_us"] = update_alone({k: opt for k, (_, opt) in steps.items()}, 100, 2 * a.rounds)
    for ts, _ in steps.values():
        ts.close()
    print("PARAM_GROUPS_TIMING_CHILD " + json.dumps(out), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256); ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=4); ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--parent-tree", default=None); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "param_groups_timing.json"))
    ap.add_argument("--child", action="store_true"); ap.add_argument("--tree", default=ROOT); ap.add_argument("--with-on", action="store_true")
    a = ap.parse_args(argv)
    if a.child:
        return child(a)
    if not a.parent_tree or not os.path.isdir(os.path.join(a.parent_tree, "raindrop_amd")):
        sys.exit("param_groups_timing: --parent-tree DIR (a built checkout of the parent commit) is required: the off path is measured against it")

    def run(tree, with_on):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", os.path.abspath(tree), "--batch", str(a.batch),
               "--block", str(a.block), "--rounds", str(a.rounds), "--warmup", str(a.warmup)] + (["--with-on"] if with_on else [])
        env = dict(os.environ)
        env.pop("RD_LIB_PATH", None)
        res = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=tree, timeout=400)
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("PARAM_GROUPS_TIMING_CHILD ")]
        if res.returncode != 0 or not line:
            sys.exit("param_groups_timing: the process on %s failed (%d):\n%s\n%s" % (tree, res.returncode, res.stdout[-2000:], res.stderr[-4000:]))
        return json.loads(line[-1][len("PARAM_GROUPS_TIMING_CHILD "):])

    parent, this_off, this_on, upd, dev, info = [], [], [], {"off": [], "on": []}, None, {}
    for pair in range(a.pairs):
        order = [("parent", a.parent_tree), ("this", ROOT)] if pair % 2 == 0 else [("this", ROOT), ("parent", a.parent_tree)]
        for name, tree in order:
            r = run(tree, name == "this")
            dev = r["device"]
            if name == "parent":
                parent.append(r["blocks"]["off"])
            else:
                this_off.append(r["blocks"]["off"]); this_on.append(r["blocks"]["on"])
                for k in upd:
                    upd[k].append(r["update_us"][k])
                info = {"groups": r["groups"], "n": r["n"], "p_drop": r["p_drop"]}
            print(name, r["blocks"], r.get("update_us"), flush=True)
    flat = lambda xs: [x for run_ in xs for x in run_]
    mean = lambda xs: sum(xs) / len(xs)
    spread = round(max(flat(parent)) - min(flat(parent)), 5)
    d_off = round(mean(flat(this_off)) - mean(flat(parent)), 5)
    res = {"workload": "TrainStep.capture_full(FlatAdam(lr=1e-4, weight_decay=%g)), P19 all-ones structure, B=%d, dropout %.1f, one hipGraph "
                       "replay per step; off: no groups (parent tree and this tree, one process each, alternating), on: "
                       "ParamGroups(flat, [no_decay(flat)]) (this tree, in the off process, alternating blocks)" % (WD, a.batch, info["p_drop"]),
           "block_steps": a.block, "rounds_per_process": a.rounds, "process_pairs": a.pairs, "warmup": a.warmup, "device": dev,
           "flat_elements": info["n"], "groups_on": info["groups"],
           "ms_per_step_blocks": {"parent_off": parent, "this_off": this_off, "this_on": this_on},
           "ms_per_step_mean": {"parent_off": round(mean(flat(parent)), 5), "this_off": round(mean(flat(this_off)), 5),
                                "this_on": round(mean(flat(this_on)), 5)},
           "margin": "off on the two trees must agree within the spread (max - min) of the parent's own blocks",
           "parent_block_spread_ms": spread, "off_this_minus_parent_ms": d_off, "off_within_parent_spread": abs(d_off) <= spread,
           "this_off_block_spread_ms": round(max(flat(this_off)) - min(flat(this_off)), 5),
           "on_minus_off_ms": round(mean(flat(this_on)) - mean(flat(this_off)), 5),
           "on_minus_off_ms_per_process": [round(mean(n) - mean(f), 5) for n, f in zip(this_on, this_off)],
           "update_launch_us": {"what": "one hipGraph of 100 x step_captured() (rd_adam_state_advance + the update), HIP events around "
                                        "a replay, per launch pair; plain = rd_adam_step_dev, grouped = rd_adam_step_grp_dev",
                                "plain": upd["off"], "grouped": upd["on"], "plain_mean": round(mean(flat(upd["off"])), 4),
                                "grouped_mean": round(mean(flat(upd["on"])), 4),
                                "grouped_minus_plain": round(mean(flat(upd["on"])) - mean(flat(upd["off"])), 4),
                                "plain_spread": round(max(flat(upd["off"])) - min(flat(upd["off"])), 4)}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
