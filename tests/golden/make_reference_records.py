"""Generate tests/golden/reference_records.npz: what the reference's OWN statements and functions return for the fixed inputs of
tests/test_feed.py and tests/test_preprocess_oracle.py, so that those tests run without the reference tree.  Where the tree is
present the tests also re-run the reference and check the record.  Run where the tree exists:

    python tests/golden/make_reference_records.py

Nothing of the reference is stored: the statements are read from `code/Raindrop.py` at run time (the index bookkeeping of its
strategy-2 batch plan, `code/Raindrop.py:261-307`), the functions imported from `code/utils_rd.py`; only their results are written.
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from oracle import ref_loader               # noqa: E402

OUT = os.path.join(HERE, "reference_records.npz")

# (record name, label seed, samples, positive rate, batch size, numpy seed, epochs): the inputs of tests/test_feed.py
FEED_CASES = [("feed_plan_b128", 5, 777, 0.07, 128, 23, 1), ("feed_epochs3_b64", 8, 900, 0.08, 64, 31, 3)]
# make_preprocess_golden.make_raw arguments of tests/test_preprocess_oracle.py's second data set
PREPROCESS_LIVE = (17, 20, 11, 7, 9)


def script_path():
    return os.path.join(ref_loader.reference_root(), "code", "Raindrop.py")


def script_available():
    return os.path.isfile(script_path())


def feed_labels(label_seed, n, rate):
    rng = np.random.default_rng(label_seed)
    return (rng.random(n) < rate).astype(np.int64)


def feed_reference_batches(ytrain, batch_size, seed, epochs):
    """The reference's own statements for the strategy-2 plan, extracted from the script and executed in its nesting: the setup
    once, then per epoch the in-place shuffles and every batch.  np.random is seeded with `seed` first.  -> [batches, batch_size]"""
    src = open(script_path()).read().splitlines()

    def grab(pat):
        hits = [ln.strip() for ln in src if re.match(pat, ln)]
        assert hits, pat
        return hits[0]
    setup = [grab(p) for p in (r"^\s*idx_0 = np\.where\(ytrain == 0\)\[0\]", r"^\s*idx_1 = np\.where\(ytrain == 1\)\[0\]",
                               r"^\s*n0, n1 = len\(idx_0\), len\(idx_1\)", r"^\s*expanded_idx_1 = np\.concatenate",
                               r"^\s*expanded_n1 = len\(expanded_idx_1\)", r"^\s*K0 = n0 //", r"^\s*K1 = expanded_n1 //",
                               r"^\s*n_batches = np\.min\(\[K0, K1\]\)")]
    per_epoch = [grab(p) for p in (r"^\s*np\.random\.shuffle\(expanded_idx_1\)", r"^\s*I1 = expanded_idx_1",
                                   r"^\s*np\.random\.shuffle\(idx_0\)", r"^\s*I0 = idx_0")]
    per_batch = [ln.strip() for ln in src if re.match(r"^\s*idx[01]_batch = I[01]\[n \* int\(batch_size / 2\)", ln)]
    assert len(per_batch) == 2
    per_batch.append(grab(r"^\s*idx = np\.concatenate\(\[idx0_batch, idx1_batch\], axis=0\)"))
    env = {"np": np, "ytrain": ytrain, "batch_size": batch_size}
    np.random.seed(seed)
    exec("\n".join(setup), env)
    out = []
    for _ in range(epochs):
        exec("\n".join(per_epoch), env)
        for n in range(int(env["n_batches"])):
            env["n"] = n
            exec("\n".join(per_batch), env)
            out.append(env["idx"].copy())
    return np.stack(out)


def preprocess_reference():
    """{name: array} of the reference's preprocessing functions on make_raw(*PREPROCESS_LIVE)."""
    import make_preprocess_golden as mk
    u = mk.ref_utils()
    arr, time, static, y = mk.make_raw(*PREPROCESS_LIVE)
    recs = [{"arr": arr[i].copy(), "time": time[i].copy(), "extended_static": static[i].copy()} for i in range(len(arr))]
    mf, stdf = u.getStats(arr.copy())
    ms, ss = u.getStats_static(static.copy(), dataset="P12")
    P, Ps, Pt, yt = u.tensorize_normalize(recs, y.copy(), mf, stdf, ms, ss)
    P2, _, Pt2, _ = u.tensorize_normalize_other(arr.copy(), y.copy(), mf, stdf)
    return {"mf": mf, "stdf": stdf, "ms": ms, "ss": ss, "P": P.numpy(), "Pstatic": Ps.numpy(), "Ptime": Pt.numpy(),
            "ytensor": yt.numpy(), "P_other": P2.numpy(), "Ptime_other": Pt2.numpy()}


def main():
    if not (ref_loader.available() and script_available()):
        raise SystemExit("reference tree not found at %s" % ref_loader.reference_root())
    out = {}
    for name, ls, n, rate, bs, seed, epochs in FEED_CASES:
        out[name] = feed_reference_batches(feed_labels(ls, n, rate), bs, seed, epochs)
    out.update(("preprocess_live/" + k, np.asarray(v)) for k, v in preprocess_reference().items())
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
