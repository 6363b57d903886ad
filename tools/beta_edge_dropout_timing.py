"""What coefficient dropout on the use_beta branch costs at the P19 benchmark shape (B = 256, 34 nodes, 1156 edges, 60 steps): the graph
operator's forward and backward launches (HIP events, median of 20 calls each, as tools/beta_timing.py) and the captured
`BetaTrainStep.capture_full(FlatAdam)` step (the model tools/bench_use_beta.py builds, dropout 0.2), at edge dropout 0 and p,
alternating.  Prints one JSON line.      python tools/beta_edge_dropout_timing.py [--batch 256] [--p 0.3] [--steps 100]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np, torch


def operator_us(B, p):
    from oracle import restatement as O2
    from raindrop_amd import ops
    n, T, d = 34, 60, 4
    K, dev = T * d, "cuda"
    rng = np.random.default_rng(0)
    ei, ew = O2.build_graph(np.ones((n, n), np.float32))
    V = torch.from_numpy(rng.standard_normal((B, n, K)).astype(np.float32)).to(dev).requires_grad_(True)
    H = torch.from_numpy(rng.standard_normal((B, n, T * 32)).astype(np.float32)).to(dev).requires_grad_(True)
    mw = torch.from_numpy(rng.standard_normal((n, 16)).astype(np.float32)).to(dev).requires_grad_(True)
    pt = torch.from_numpy(rng.standard_normal((B, T, 16)).astype(np.float32)).to(dev)
    R = torch.from_numpy(rng.standard_normal((B, n, K)).astype(np.float32)).to(dev)
    eid, ewd = torch.from_numpy(ei).to(dev), torch.from_numpy(ew).to(dev).reshape(1, -1)
    out = {}
    for pp in (0.0, p, 0.0, p):
        tf, tb = [], []
        for it in range(23):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            Y, _, _ = ops.graph_beta(V, H, mw, pt, eid, ewd, d, p_drop=pp, seed=it)
            e[1].record()
            torch.autograd.grad((Y * R).sum(), [V, H, mw])
            e[2].record(); torch.cuda.synchronize()
            if it >= 3:
                tf.append(e[0].elapsed_time(e[1]) * 1e3); tb.append(e[1].elapsed_time(e[2]) * 1e3)
        out.setdefault("p=%g" % pp, []).append({"fwd_us": round(float(np.median(tf)), 1),
                                                "bwd_us_incl_the_loss_kernels": round(float(np.median(tb)), 1)})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256); ap.add_argument("--p", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=100); ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args(argv)
    from bench_use_beta import build
    from raindrop_amd import dp, synth
    from raindrop_amd.optim import FlatAdam
    from raindrop_amd.step_beta import BetaTrainStep
    dev = torch.device("cuda", 0)
    res = {"workload": "P19 all-ones structure, B=%d" % a.batch, "p": a.p, "operator": operator_us(a.batch, a.p)}
    steps = {}
    for pe in (0.0, a.p):
        cfg, m, b = build(a.batch, dev)
        m.ob_propagation.dropout = pe
        named = dict(m.named_parameters())
        flat = dp.FlatGradAllReduce([(n, named[n]) for n in synth.live_parameter_names_beta(cfg)], n_buckets=2)
        opt = FlatAdam(flat.flatten_parameters(), lr=1e-4)                   # (before the step: it moves the parameters)
        st = BetaTrainStep(m, flat, b)
        st.capture_full(opt)
        steps["edge_p=%g" % pe] = st
    times = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, st in steps.items():
            for _ in range(a.warmup):
                st.run_full()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.steps):
                st.run_full()
            torch.cuda.synchronize()
            times[k].append(round((time.perf_counter() - t0) / a.steps * 1e3, 4))
    res["BetaTrainStep_ms_per_step"] = times
    for st in steps.values():
        st.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
