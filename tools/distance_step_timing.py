"""Cost of the structure-distance regulariser in the captured use_beta step: AutogradStep at P19 (all-ones structure, Kk = 578
kept edges per sample), B = 256, dropout 0.2, once with distance_weight = 0 (CE alone) and once with lambda != 0 (CE + lambda *
distance: rd_structure_distance_bwd + the alpha cotangent of rd_graph_beta_bwd_alpha), in one process.  Prints one JSON line.

    python tools/distance_step_timing.py [--batch 256] [--steps 50] [--warmup 10] [--lam 1e-4]

Under `rocprofv3 --kernel-trace --stats -- python tools/distance_step_timing.py` the kernel statistics carry both steps: the
new / changed kernels (k_graph_beta_bwd2<true>, k_distance_coef, k_distance_bwd) appear in the lambda != 0 step only."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256); ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10); ap.add_argument("--lam", type=float, default=1e-4)
    a = ap.parse_args(argv)
    from bench_use_beta import build
    from raindrop_amd.step import AutogradStep
    dev = torch.device("cuda", 0)
    res = {}
    for lam in (0.0, a.lam):
        cfg, m, b = build(a.batch, dev)
        st = AutogradStep(m, b, lr=1e-4, distance_weight=lam)
        for _ in range(a.warmup):
            st.run()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = st.run()
        torch.cuda.synchronize(); t1 = time.perf_counter()
        assert bool(torch.isfinite(loss))
        res["lam=%g" % lam] = {"ms_per_step": round((t1 - t0) * 1e3 / a.steps, 4), "loss": float(loss), "distance": float(st.distance)}
        st.close()
        del st, m
    print(json.dumps({"workload": "AutogradStep, P19 all-ones structure, Raindrop_v2(use_beta=True, compute_distance=True), B=%d, "
                                  "dropout 0.2, fwd+loss+bwd+Adam" % a.batch, "steps": a.steps, "warmup": a.warmup, **res}), flush=True)


if __name__ == "__main__":
    main()
