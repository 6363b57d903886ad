"""Cost of the focal loss in the whole-step graph: TrainStep.capture_full at P19, B = 256 (the model, batch, structure and optimizer
of bench.py), three steps in ONE process -- the plain mean cross entropy (the launches of a tree without the feature), the weighted
criterion TrainStep(class_weight=[1, 6]) (rd_head_train_crit) and TrainStep(class_weight=[1, 6], focal_gamma=2) (rd_head_train_focal) --
timed in alternating blocks of `--block` replays (wall clock around a synchronize), so that clocks and neighbours are shared.  Writes
one JSON object (`--bench-ab FILE`: merged under the key "bench_ab", the focal_gamma=None A/B of bench.py against the parent commit
recorded beside it).

    python tools/focal_loss_timing.py [--batch 256] [--block 100] [--rounds 6] [--warmup 30] [--out profiles/focal_loss_timing.json]
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from tools.ce_criterion_timing import build


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256); ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=6); ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--bench-ab", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "focal_loss_timing.json"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    made = {"plain": build(a.batch, dev), "class_weight": build(a.batch, dev, class_weight=[1.0, 6.0]),
            "focal": build(a.batch, dev, class_weight=[1.0, 6.0], focal_gamma=2.0)}
    steps = {k: v[0] for k, v in made.items()}
    assert steps["plain"].crit is None and steps["plain"].focal is None and steps["class_weight"].crit is not None
    assert steps["focal"].focal is not None and steps["focal"].crit is None and steps["focal"].head_fused
    for k, (ts, opt) in made.items():
        ts.capture_full(opt)
    for ts in steps.values():
        for _ in range(a.warmup):
            ts.run_full()
    torch.cuda.synchronize()
    blocks = {k: [] for k in steps}
    for _ in range(a.rounds):
        for name, ts in steps.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.block):
                loss = ts.run_full()
            torch.cuda.synchronize(); t1 = time.perf_counter()
            assert bool(torch.isfinite(loss))
            blocks[name].append(round((t1 - t0) * 1e3 / a.block, 5))
    mean = {k: sum(v) / len(v) for k, v in blocks.items()}
    res = {"workload": "TrainStep.capture_full(FlatAdam(lr=1e-4)), P19 all-ones structure, B=%d, dropout %.1f, one hipGraph replay per "
                       "step; plain: mean cross entropy, class_weight: class_weight=[1, 6], focal: class_weight=[1, 6], focal_gamma=2"
                       % (a.batch, steps["plain"].p_drop),
           "block_steps": a.block, "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "ms_per_step_blocks": blocks, "ms_per_step_mean": {k: round(v, 5) for k, v in mean.items()},
           "block_spread_ms": {k: round(max(v) - min(v), 5) for k, v in blocks.items()},
           "focal_minus_class_weight_ms": round(mean["focal"] - mean["class_weight"], 5),
           "focal_minus_plain_ms": round(mean["focal"] - mean["plain"], 5),
           "steps_taken": {k: v[1].t for k, v in made.items()}}
    if a.bench_ab:
        with open(a.bench_ab) as fh:
            res["bench_ab"] = json.load(fh)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res), flush=True)
    for ts in steps.values():
        ts.close()


if __name__ == "__main__":
    main()
