"""The two captured training steps of the paper's branch side by side, in one process: `AutogradStep` (the module's autograd surface
replayed, torch's Adam inside the graph) against `BetaTrainStep.capture_full(FlatAdam)` (the hand-enqueued step: rd_beta_stage_fwd /
_bwd, the fused encoder chains, the fused head + loss, the token plan, one Adam kernel).  P19 shape, all-ones structure (the model
tools/bench_use_beta.py builds), dropout 0.2, both steps fwd + CE + bwd + Adam.  Timed alternately -- A B A B, the same warm-up and
step counts for every block -- so that clock drift hits both alike.  Prints one JSON line.

    python tools/beta_step_timing.py [--batch 256] [--steps 100] [--warmup 20] [--rounds 2]

Under `rocprofv3 --kernel-trace --stats -- python tools/beta_step_timing.py` the kernel statistics carry both steps."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256); ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20); ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args(argv)
    from bench_use_beta import build
    from raindrop_amd import dp, synth
    from raindrop_amd.optim import FlatAdam
    from raindrop_amd.step import AutogradStep
    from raindrop_amd.step_beta import BetaTrainStep
    dev = torch.device("cuda", 0)
    cfg, ma, ba = build(a.batch, dev)
    auto = AutogradStep(ma, ba, lr=1e-4)
    cfg, mb, bb = build(a.batch, dev)
    named = dict(mb.named_parameters())
    flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names_beta(cfg)], n_buckets=2)
    opt = FlatAdam(flat.flatten_parameters(), lr=1e-4)
    beta = BetaTrainStep(mb, flat, bb)
    beta.capture_full(opt)
    runs = {"AutogradStep": auto.run, "BetaTrainStep": beta.run_full}
    times = {k: [] for k in runs}
    loss = {}
    for _ in range(a.rounds):                                     # A B A B
        for name, fn in runs.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.steps):
                l = fn()
            torch.cuda.synchronize(); t1 = time.perf_counter()
            assert bool(torch.isfinite(l)), name
            times[name].append(round((t1 - t0) * 1e3 / a.steps, 4))
            loss[name] = float(l)
    best = {k: min(v) for k, v in times.items()}
    print(json.dumps({"workload": "P19 all-ones structure, Raindrop_v2(use_beta=True, compute_distance=True), B=%d, dropout 0.2, "
                                  "fwd+CE+bwd+Adam, one hipGraph per step each" % a.batch, "steps": a.steps, "warmup": a.warmup,
                      "order": "alternating, %d rounds" % a.rounds, "ms_per_step": times, "best_ms_per_step": best,
                      "speedup": round(best["AutogradStep"] / best["BetaTrainStep"], 3), "loss": loss,
                      "token_plan": beta.plan is not None, "tuned": [beta.tuned_rows32, beta.tuned_waves16]}), flush=True)
    auto.close(); beta.close()


if __name__ == "__main__":
    main()
